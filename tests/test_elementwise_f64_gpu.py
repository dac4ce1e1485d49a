"""The loss, reduction and layout kernels as direct calls, on every dispatch form, grid trip and edge: cast, axpy,
scale_cast, patchify, colsum (direct fold, rows-per-workgroup, 4-wide and scalar partial kernels, the fold queue) and
softmax_xent (csrc/elementwise.hip), gelu_fwd / gelu_bwd (csrc/split3.hip), colsum_mul (csrc/cait_ops.hip),
relpos gather / scatter, patch_merge and token_mean (csrc/swin_ops.hip).  References, inputs and case lists:
tests/elementwise_util.py (float64 or integer torch on the CPU); tests/test_elementwise_ref_cpu.py checks them and
measures the bounds below.  Every check prints its error beside its bound (-s); every output is carved out of a buffer
pre-filled with NaN (integers: a sentinel), so an unwritten element fails its check and a store outside the output
fails the guard check.

1. Exact sections.  Operands are integers in [-8, 8]: every partial and final sum is an integer below 2^24, exact in
   fp32 in any order, and the result must equal the integer reference bit for bit (a dropped, doubled or misplaced row,
   column group or trip is off by at least 1).  The pure copies (cast, patchify, patch_merge, relpos gather,
   token_mean_bwd, scale_cast: IEEE multiplies in a fixed order and one rounding) are bitwise on arbitrary values; a NaN
   equals any NaN.  Printed: the number of differing elements, bound 0.
2. Accuracy sections, normal inputs against float64.
   * sums (colsum, colsum_mul, token_mean_fwd, relpos_scatter): per output element |got - want| / sum |terms of that
     element|, the maximum over elements.  Bound: 4x the same metric of the same sum in torch float32 on the CPU over
     the section's inputs (the factor covers another summation order):
       colsum 1.70e-8 [GPU 1.50e-8], colsum_mul 1.41e-8 [1.09e-8], token_mean_fwd 3.98e-8 [1.07e-7],
       relpos_scatter 1.73e-7 [1.72e-7]
   * axpy: per element |got - want| <= 2^-23 (|y| + |a x|), fused or not.  Printed: the largest error / bound [0.50].
   * gelu_fwd, gelu_bwd (|dh| <= 1): |got - want| / max(1, |x|) per element.  Bound: 4x the same metric of torch's
     float32 CPU F.gelu and its autograd on these inputs: fwd 3.80e-7 [GPU 1.20e-7], bwd 2.57e-7 [1.68e-7].
3. softmax_xent against float64 log_softmax: loss[0], every loss[1 + b] (relative to max(1, |loss_b|)), all of dlogits
   (relative to 1 / B), correct[0] and every correct[1 + b] (exact).  Bound: 4x the error of torch's float32 CPU
   cross_entropy and its autograd over all the valid-label cases here: loss 1.99e-7 [GPU 4.68e-7], dlogits 3.14e-7
   [6.18e-7].  The kernel forms lse = max + log(sum) and takes the loss and every gradient's exponential from it; at
   logits shifted by +-3e4 that rounds log(sum) to 2^-9 (it measured loss 7.99e-4, dlogits 7.09e-4 against these
   bounds).  Rows with |lse| >= 16 are now worked relative to their maximum (the shifted cases: 9.8e-8, 1.1e-7); below
   16 the arithmetic and its bits are unchanged, and two shifts put rows of one batch on either side of the switch.
"""
import functools
import math

import pytest
import torch

import elementwise_util as U
from elementwise_util import BF16, F32, F64

pytestmark = pytest.mark.gpu

# torch float32 on the CPU against float64 over each section's inputs (tests/test_elementwise_ref_cpu.py measures them
# again and asserts these are not below what it finds); the bounds are 4x these
F32_COLSUM = 1.70e-8
F32_COLSUM_MUL = 1.41e-8
F32_TOKEN_MEAN = 3.98e-8
F32_RELPOS_SCATTER = 1.73e-7
F32_GELU = {"fwd": 3.80e-7, "bwd": 2.57e-7}
F32_XENT = {"loss": 1.99e-7, "dlogits": 3.14e-7}
FACTOR = 4.0

GUARD = 1024                   # elements of sentinel on either side of a carved output
INT_SENTINEL = -777


@pytest.fixture(scope="module")
def ops(lib):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from vit_torch_amd import ops as _ops
    return _ops


def carve(shape, dtype):
    """(buffer, output): the output is a contiguous view GUARD elements into a buffer of NaN (integers: the sentinel)."""
    n = math.prod(shape)
    fill = float("nan") if dtype.is_floating_point else INT_SENTINEL
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(name, buf, out):
    torch.cuda.synchronize()
    g = torch.cat([buf[:GUARD], buf[GUARD + out.numel():]])
    ok = torch.isnan(g).all() if g.is_floating_point() else (g == INT_SENTINEL).all()
    assert bool(ok), f"{name}: a store outside the output"


def exact(name, got, want):
    """Bit for bit; prints the number of differing elements beside its bound, 0."""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {got.dtype} {tuple(got.shape)}"
    if got.is_floating_point():
        gn, wn = torch.isnan(got), torch.isnan(want)
        diff = (gn != wn) | ((U.bits(got) != U.bits(want)) & ~(gn & wn))
    else:
        diff = got != want
    n = int(diff.sum())
    print(f"\n  {name}: {n} of {got.numel()} elements differ (0)", end="")
    if n:
        at = diff.reshape(-1).nonzero()[0].item()
        raise AssertionError(f"{name}: {n} of {got.numel()} elements differ, the first at flat index {at}: got "
                             f"{got.reshape(-1)[at].item()!r}, want {want.reshape(-1)[at].item()!r}")


def within(name, errs, bounds):
    print(f"\n  {name}: " + "  ".join(f"{k} {v:.2e} ({bounds[k]:.1e})" for k, v in errs.items()), end="")
    bad = {k: (v, bounds[k]) for k, v in errs.items() if not v <= bounds[k]}
    assert not bad, f"{name}: over the bound: {bad}"


# ===================================================================================== 1. exact sections ========
# ------------------------------------------------------------------------------------------------------ colsum ---
def run_colsum(ops, c, values, **kw):
    x = c.view(values.to(c.dtype).cuda())
    buf, out = carve((c.N,), F32)
    ops.colsum(x, out, M=c.M, N=c.N, ld=c.ld, **kw)
    return buf, out


@pytest.mark.parametrize("c", U.colsum_cases(), ids=lambda c: c.id)
def test_colsum_exact(ops, c):
    vals = c.integers()
    buf, out = run_colsum(ops, c, vals)
    guards_intact(c.id, buf, out)
    exact(f"colsum {c.id}", out, c.view(vals).sum(0).to(F32))


def test_colsum_fold_queue_exact(ops):
    """A queued fold of a short fp32 matrix runs at flush() and equals the immediate call bit for bit."""
    M, N = U.FOLD_QUEUE_CASE
    c = U.ColsumCase("direct", F32, M, N)
    vals = c.integers()
    _, now = run_colsum(ops, c, vals)
    q = ops.FoldQueue()
    buf, later = run_colsum(ops, c, vals, fold=q)
    torch.cuda.synchronize()
    assert len(q) == 1 and bool(torch.isnan(later).all()), "the queued fold must not run before flush()"
    q.flush()
    guards_intact("fold queue", buf, later)
    assert len(q) == 0
    exact("colsum fold queue vs immediate", later, now.cpu())
    exact("colsum fold queue", later, c.view(vals).sum(0).to(F32))


# -------------------------------------------------------------------------------------------------- colsum_mul ---
@pytest.mark.parametrize("M,N,ldx,ldy", U.COLSUM_MUL_SHAPES, ids=lambda v: str(v))
def test_colsum_mul_exact(ops, M, N, ldx, ldy):
    xi, yi = U.colsum_mul_integers(M, N, ldx, ldy)
    want = (xi[:, :N] * yi[:, :N]).sum(0).to(F32)
    for (xdt, ydt), pid in zip(U.PAIRS, U.PAIR_IDS):
        buf, out = carve((N,), F32)
        ops.colsum_mul(xi.to(xdt).cuda(), yi.to(ydt).cuda(), out, M=M, N=N, ldx=ldx, ldy=ldy)
        guards_intact(pid, buf, out)
        exact(f"colsum_mul M{M} N{N} {pid}", out, want)


# -------------------------------------------------------------------------------------------------- token mean ---
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,L,C", U.TOKEN_MEAN_FWD)
def test_token_mean_fwd_exact(ops, B, L, C, dt):
    xi = U.ints((B, L, C), 10 * L)
    buf, out = carve((B, C), F32)
    ops.token_mean_fwd(xi.to(dt).cuda(), out, B, L, C)
    guards_intact("token_mean_fwd", buf, out)
    exact(f"token_mean_fwd L{L} {U.DT_NAME[dt]}", out, U.token_mean_exact(xi))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_token_mean_bwd_exact(ops, dt):
    B, L, C = U.TOKEN_MEAN_BWD
    dout = U.normal((B, C), 11)
    buf, dx = carve((B, L, C), dt)
    ops.token_mean_bwd(dout.cuda(), dx, B, L, C)
    guards_intact("token_mean_bwd", buf, dx)
    exact(f"token_mean_bwd {U.DT_NAME[dt]}", dx, U.token_mean_bwd_ref(dout, L, dt, B))


# ------------------------------------------------------------------------------------------------------ relpos ---
@pytest.mark.parametrize("ws,H", U.RELPOS_CASES)
def test_relpos_gather_scatter_exact(ops, ws, H):
    N, T = ws * ws, (2 * ws - 1) ** 2
    idx = U.relpos_index(ws)
    table = U.normal((T, H), ws + H)
    buf, bias = carve((H, N, N), F32)
    ops.relpos_bias_gather(table.cuda(), idx.cuda(), bias, T, H, N)
    guards_intact("relpos gather", buf, bias)
    exact(f"relpos gather ws{ws} H{H}", bias, U.relpos_gather_ref(table, idx))
    dbi = U.ints((H, N, N), ws + H + 1)
    buf, dtable = carve((T, H), F32)
    ops.relpos_bias_scatter(dbi.to(F32).cuda(), idx.cuda(), dtable, T, H, N)
    guards_intact("relpos scatter", buf, dtable)
    exact(f"relpos scatter ws{ws} H{H}", dtable, U.relpos_scatter_ref(dbi, idx, T).to(F32))


# -------------------------------------------------------------------------------------------------------- cast ---
@pytest.mark.parametrize("sdt,ddt", U.PAIRS, ids=U.PAIR_IDS)
def test_cast_exact(ops, sdt, ddt):
    x = U.cast_input(sdt)
    buf, out = carve((U.CAST_N,), ddt)
    ops.cast(x.cuda(), out)
    guards_intact("cast", buf, out)
    exact(f"cast {U.DT_NAME[sdt]}->{U.DT_NAME[ddt]}", out, x.to(ddt))


# ---------------------------------------------------------------------------------------------------- patchify ---
@functools.lru_cache(maxsize=None)
def patchify_image():
    B, C, H, p, cls = U.PATCHIFY_CASE
    return U.normal((B, C, H, H), 21)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("odt,ld", [(F32, None), (BF16, None), (BF16, U.PATCHIFY_PAD_LD)], ids=["fp32", "bf16", "bf16-padded"])
def test_patchify_exact(ops, odt, ld, channels_last):
    B, C, H, p, cls = U.PATCHIFY_CASE
    x = patchify_image()
    xd = x.cuda()
    if channels_last:
        xd = xd.contiguous(memory_format=torch.channels_last)
    want = U.patchify_ref(x, p, cls, ld).to(odt)
    buf, out = carve(tuple(want.shape), odt)
    ops.patchify(xd, out, p, cls)
    guards_intact("patchify", buf, out)
    exact(f"patchify {U.DT_NAME[odt]} ld {ld}", out, want)


# ------------------------------------------------------------------------------------------------- patch merge ---
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,Hh,Ww,C", U.PATCH_MERGE_CASES)
def test_patch_merge_exact(ops, B, Hh, Ww, C, dt):
    x = U.normal((B, Hh * Ww, C), Hh + C).to(dt)
    want = U.patch_merge_ref(x, B, Hh, Ww, C)
    buf, out = carve(tuple(want.shape), dt)
    ops.patch_merge(x.cuda(), out, B, Hh, Ww, C)
    guards_intact("patch_merge", buf, out)
    exact(f"patch_merge {Hh}x{Ww} {U.DT_NAME[dt]}", out, want)
    buf, back = carve(tuple(x.shape), dt)
    ops.patch_merge(want.cuda(), back, B, Hh, Ww, C, inverse=True)
    guards_intact("patch_merge inverse", buf, back)
    exact(f"patch_merge inverse {Hh}x{Ww} {U.DT_NAME[dt]}", back, x)


# -------------------------------------------------------------------------------------------------- scale_cast ---
@pytest.mark.parametrize("form", list(U.SCALE_FORMS))
@pytest.mark.parametrize("xdt,odt", U.PAIRS, ids=U.PAIR_IDS)
def test_scale_cast_exact(ops, xdt, odt, form):
    M, N, rpg = U.SCALE_CAST_SHAPE
    ldx, ldo = U.SCALE_CAST_LDX, U.SCALE_CAST_LDO
    x, col, row = U.scale_cast_inputs(xdt)
    use_col, use_row = U.SCALE_FORMS[form]
    want = U.scale_cast_ref(x[:, :N], col if use_col else None, row if use_row else None, rpg, odt)
    kw = dict(M=M, N=N, rowscale=row.cuda() if use_row else None, rows_per_group=rpg if use_row else 0)
    cold = col.cuda() if use_col else None
    name = f"scale_cast {U.DT_NAME[xdt]}->{U.DT_NAME[odt]} {form}"
    buf, out = carve((M, N), odt)
    ops.scale_cast(x[:, :N].contiguous().cuda(), out, cold, **kw)
    guards_intact(name, buf, out)
    exact(name, out, want)
    # rows at larger strides on both sides: the columns past N keep their NaN
    buf, wide = carve((M, ldo), odt)
    ops.scale_cast(x.cuda(), wide, cold, ldx=ldx, ldo=ldo, **kw)
    guards_intact(name + " strided", buf, wide)
    exact(name + " strided", wide[:, :N], want)
    assert bool(torch.isnan(wide[:, N:]).all()), f"{name}: a column past N was written"


def test_scale_cast_in_place_exact(ops):
    """out is x (fp32 -> fp32): how DDP scales a gradient bucket."""
    M, N, rpg = U.SCALE_CAST_SHAPE
    x, col, row = U.scale_cast_inputs(F32)
    buf, io = carve((M, N), F32)
    io.copy_(x[:, :N])
    ops.scale_cast(io, io, col.cuda(), M=M, N=N, rowscale=row.cuda(), rows_per_group=rpg)
    guards_intact("scale_cast in place", buf, io)
    exact("scale_cast in place", io, U.scale_cast_ref(x[:, :N], col, row, rpg, F32))


# ================================================================================== 2. accuracy sections ========
@pytest.mark.parametrize("c", U.colsum_accuracy_cases(), ids=lambda c: c.id)
def test_colsum_against_float64(ops, c):
    vals = c.normals().to(c.dtype)
    buf, out = run_colsum(ops, c, vals)
    guards_intact(c.id, buf, out)
    x = c.view(vals).to(F64)
    within(f"colsum {c.id}", {"sum": U.sum_metric(out.cpu(), x.sum(0), x.abs().sum(0))}, {"sum": FACTOR * F32_COLSUM})


@pytest.mark.parametrize("xdt,ydt", U.PAIRS, ids=U.PAIR_IDS)
def test_colsum_mul_against_float64(ops, xdt, ydt):
    M, N, ldx, ldy = U.COLSUM_MUL_ACCURACY
    x, y = U.colsum_mul_normals(M, N, ldx, ldy)
    x, y = x.to(xdt), y.to(ydt)
    buf, out = carve((N,), F32)
    ops.colsum_mul(x.cuda(), y.cuda(), out, M=M, N=N, ldx=ldx, ldy=ldy)
    guards_intact("colsum_mul", buf, out)
    prod = x.to(F64) * y.to(F64)
    within(f"colsum_mul {U.DT_NAME[xdt]}-{U.DT_NAME[ydt]}", {"sum": U.sum_metric(out.cpu(), prod.sum(0), prod.abs().sum(0))},
           {"sum": FACTOR * F32_COLSUM_MUL})


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_token_mean_fwd_against_float64(ops, dt):
    B, L, C = U.TOKEN_MEAN_ACCURACY
    x = U.token_mean_accuracy_input(dt)
    buf, out = carve((B, C), F32)
    ops.token_mean_fwd(x.cuda(), out, B, L, C)
    guards_intact("token_mean_fwd", buf, out)
    e = U.sum_metric(out.cpu(), x.to(F64).mean(1), x.to(F64).abs().sum(1) / L)
    within(f"token_mean_fwd {U.DT_NAME[dt]}", {"mean": e}, {"mean": FACTOR * F32_TOKEN_MEAN})


def test_relpos_scatter_against_float64(ops):
    ws, H = U.RELPOS_ACCURACY
    N, T = ws * ws, (2 * ws - 1) ** 2
    idx, db = U.relpos_index(ws), U.relpos_accuracy_input()
    buf, dtable = carve((T, H), F32)
    ops.relpos_bias_scatter(db.cuda(), idx.cuda(), dtable, T, H, N)
    guards_intact("relpos scatter", buf, dtable)
    e = U.sum_metric(dtable.cpu(), U.relpos_scatter_ref(db.to(F64), idx, T), U.relpos_scatter_ref(db.to(F64).abs(), idx, T))
    within("relpos scatter", {"sum": e}, {"sum": FACTOR * F32_RELPOS_SCATTER})


@pytest.mark.parametrize("a", U.AXPY_A)
def test_axpy_against_float64(ops, a):
    x, y = U.axpy_inputs()
    buf, io = carve((U.AXPY_N,), F32)
    io.copy_(y)
    ops.axpy(x.cuda(), io, a)
    guards_intact("axpy", buf, io)
    want, bound = U.axpy_ref(x, y, a)
    got = io.cpu()
    assert bool(torch.isfinite(got).all())
    ratio = ((got.to(F64) - want).abs() / bound).max().item()
    within(f"axpy a = {a}", {"error / (2^-23 (|y| + |a x|))": ratio}, {"error / (2^-23 (|y| + |a x|))": 1.0})


def gelu_bounds():
    return {k: FACTOR * v for k, v in F32_GELU.items()}


def test_gelu_past_the_grid_cap_against_float64(ops):
    M, N = U.GELU_BIG
    pre, dh = U.gelu_inputs(M, N, 31)
    wy, wg = U.gelu_ref(pre, dh)
    by, y = carve((M, N), F32)
    bg, g = carve((M, N), F32)
    ops.gelu_fwd(pre.cuda(), y)
    ops.gelu_bwd(dh.cuda(), pre.cuda(), g)
    guards_intact("gelu_fwd", by, y)
    guards_intact("gelu_bwd", bg, g)
    y, g = y.cpu(), g.cpu()
    assert bool(torch.isfinite(y).all() and torch.isfinite(g).all())
    within("gelu 2112 x 2048", {"fwd": U.gelu_metric(y, wy, pre), "bwd": U.gelu_metric(g, wg, pre)}, gelu_bounds())


def test_gelu_three_row_strides_against_float64(ops):
    """ldp, ldd and ldo all different and larger than N; the input padding is NaN, the output padding must stay NaN."""
    M, N, ldp, ldd, ldo = U.GELU_SMALL
    pre, dh = U.gelu_inputs(M, N, 33)
    wy, wg = U.gelu_ref(pre, dh)

    def padded(t, ld):
        b = torch.full((M, ld), float("nan"), device="cuda")
        b[:, :N] = t.cuda()
        return b[:, :N]
    by, y = carve((M, ldo), F32)
    bg, g = carve((M, ldo), F32)
    ops.gelu_fwd(padded(pre, ldp), y[:, :N])
    ops.gelu_bwd(padded(dh, ldd), padded(pre, ldp), g[:, :N])
    guards_intact("gelu_fwd", by, y)
    guards_intact("gelu_bwd", bg, g)
    assert bool(torch.isnan(y[:, N:]).all() and torch.isnan(g[:, N:]).all()), "a column past N was written"
    y, g = y[:, :N].cpu(), g[:, :N].cpu()
    assert bool(torch.isfinite(y).all() and torch.isfinite(g).all())
    within("gelu 5 x 12 strided", {"fwd": U.gelu_metric(y, wy, pre), "bwd": U.gelu_metric(g, wg, pre)}, gelu_bounds())


# ========================================================================================= 3. softmax_xent ========
def run_xent(ops, logits, labels):
    B, K = logits.shape
    bl, loss = carve((1 + B,), F32)
    bc, correct = carve((1 + B,), torch.int32)
    bd, dl = carve((B, K), F32)
    ops.softmax_xent(logits.cuda(), labels.cuda(), loss, dl, correct)
    guards_intact("xent loss", bl, loss)
    guards_intact("xent correct", bc, correct)
    guards_intact("xent dlogits", bd, dl)
    return loss.cpu(), dl.cpu(), correct.cpu()


def xent_bounds():
    return {k: FACTOR * v for k, v in F32_XENT.items()}


def judge_xent(name, got, want):
    loss, dl, correct = got
    assert bool(torch.isfinite(dl).all()), f"{name}: non-finite dlogits"
    within(f"xent {name}", U.xent_errors(loss, dl, want), xent_bounds())
    exact(f"xent {name} correct", correct, want.correct)


@pytest.mark.parametrize("B,K", U.xent_sweep_cases())
def test_xent_batch_and_class_sweep(ops, B, K):
    logits, labels = U.xent_sweep_inputs(B, K)
    got = run_xent(ops, logits, labels)
    assert bool(torch.isfinite(got[0]).all())
    judge_xent(f"B{B} K{K}", got, U.XentRef(logits, labels))


def test_xent_tied_maxima_count_the_lowest_index(ops):
    logits, labels, ties = U.xent_tie_inputs()
    want = U.XentRef(logits, labels)
    got = run_xent(ops, logits, labels)
    judge_xent("ties", got, want)
    for b, idx in enumerate(ties):
        assert got[2][1 + b].item() == int(labels[b].item() == idx[0]), f"row {b}: ties at {idx}, label {labels[b].item()}"


def test_xent_logits_scaled_until_all_but_one_exponential_underflows(ops):
    logits, labels = U.xent_scale_inputs()
    big = logits * 1e4
    got = run_xent(ops, big, labels)
    assert bool(torch.isfinite(got[0]).all())
    judge_xent("x 1e4", got, U.XentRef(big, labels))


@pytest.mark.parametrize("shift", [U.XENT_SHIFT, -U.XENT_SHIFT, *U.XENT_SWITCH_SHIFTS], ids=["plus3e4", "minus3e4", "plus10", "minus21p5"])
def test_xent_shifted_logits_match_the_unshifted_answers(ops, shift):
    logits, labels = U.xent_scale_inputs()
    want = U.XentRef(logits, labels)
    judge_xent("unshifted", run_xent(ops, logits, labels), want)
    judge_xent(f"shifted by {shift:+.0e}", run_xent(ops, logits + shift, labels), want)


def test_xent_minus_infinity_logit_has_zero_gradient(ops):
    logits, labels, at = U.xent_neginf_inputs()
    got = run_xent(ops, logits, labels)
    assert bool(torch.isfinite(got[0]).all())
    judge_xent("-inf logit", got, U.XentRef(logits, labels))
    g = got[1][torch.arange(logits.shape[0]), at]
    assert bool((U.bits(g) == 0).all()), f"the gradient at a -inf logit must be +0: {g}"


def test_xent_out_of_range_labels(ops):
    """The kernel's contract (xent_kernel): a label outside [0, K) never becomes an out-of-bounds read; its sample's
    loss and with it the mean are NaN, it counts as incorrect, and its dlogits row is softmax / B (no class matches)."""
    logits, labels, bad = U.xent_bad_label_inputs()
    want = U.XentRef(logits, labels)
    loss, dl, correct = got = run_xent(ops, logits, labels)
    assert math.isnan(loss[0].item()) and all(math.isnan(loss[1 + b].item()) for b in bad)
    good = [b for b in range(logits.shape[0]) if b not in bad]
    assert bool(torch.isfinite(loss[1:][good]).all())
    assert all(correct[1 + b].item() == 0 for b in bad)
    judge_xent("bad labels", got, want)                       # every other row's loss and count, all of dlogits
    sm = torch.softmax(logits.to(F64), -1) / logits.shape[0]
    within("xent bad rows' dlogits vs softmax / B",
           {"dlogits": ((dl.to(F64) - sm)[bad].abs().max() * logits.shape[0]).item()}, xent_bounds())
