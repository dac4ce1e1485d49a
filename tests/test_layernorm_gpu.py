"""LayerNorm (csrc/layernorm.hip) as direct calls against float64: every (LPR, NV) form of the 8-element kernels, the
4-element kernels (D % 8 == 4, strides that are no multiple of 8, the vitmi_debug_ln8(0) hook), every dtype combination
built, the grid-stride row loops, padded strides with sentinel guards, the branch scales, degenerate rows, determinism,
the forward -> backward round trip and the refusals.

The inputs, references, bounds and case tables are tests/ln_util.py's; tests/test_layernorm_cpu.py proves on the host that
the tables reach what they claim and that the bounds leave the fp32 arithmetic itself a factor of two.  Checks are
element-wise in the units ln_util.BOUNDS documents, never relative to the largest element of the result."""
import pytest
import torch

import ln_util as U
from ln_util import DT, Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(lib):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from vit_torch_amd import ops as _ops
    return _ops


def dev(t):
    return None if t is None else t.to(device="cuda", dtype=torch.float32).contiguous()


class hook_off:
    """vitmi_debug_ln8(0) for the calls inside: the 4-element kernels everywhere."""

    def __init__(self, lib, active=True):
        self.lib, self.active = lib, active

    def __enter__(self):
        if self.active:
            self.lib.vitmi_debug_ln8(0)

    def __exit__(self, *exc):
        if self.active:
            self.lib.vitmi_debug_ln8(1)
        return False


# ------------------------------------------------------------------------------------------------ runners ---
def run_fwd(ops, lib, c, inp, force4=None):
    x = Guarded(c.M, c.D, DT[c.xdt], "cuda", c.xs, inp["x"])
    y = Guarded(c.M, c.D, DT[c.ydt], "cuda", c.ys)
    mean, rstd = Guarded(1, c.M, torch.float32, "cuda"), Guarded(1, c.M, torch.float32, "cuda")
    with hook_off(lib, c.force4 if force4 is None else force4):
        ops.layernorm_fwd(x.win, dev(inp["gamma"]), dev(inp["beta"]), y.win, mean.win, rstd.win, c.eps, M=c.M, D=c.D,
                          x_stride=x.stride, y_stride=y.stride)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, rstd=rstd)


def check_fwd(c, inp, out):
    for k in ("y", "mean", "rstd"):
        assert out[k].intact(), f"{c.id}: something outside {k}'s M x D window was written"
    y, mean, rstd = out["y"].cpu(), out["mean"].cpu()[0], out["rstd"].cpu()[0]
    for r0 in range(0, c.M, U.ROW_CHUNK):                       # the float64 reference a block of rows at a time
        r1 = min(c.M, r0 + U.ROW_CHUNK)
        x = inp["x"][r0:r1]
        wy, wm, wr = U.ref_fwd(x, inp["gamma"], inp["beta"], c.eps)
        sy, sm = U.fwd_scales(x, inp["beta"])
        U.check("y", c.data, y[r0:r1], wy, sy)
        U.check("mean", c.data, mean[r0:r1], wm, sm)
        U.check("rstd", c.data, rstd[r0:r1], wr, wr)
    return y, mean, rstd


def run_bwd(ops, lib, c, inp, force4=None, fold=None, mean=None, rstd=None):
    dy = Guarded(c.M, c.D, DT[c.dy], "cuda", c.dys, inp["dy"])
    x = Guarded(c.M, c.D, DT[c.r], "cuda", c.xs, inp["x"])
    g_in = Guarded(c.M, c.D, DT[c.r], "cuda", c.gs, inp["g_in"]) if c.g_in else None
    g_out = g_in if c.inplace else Guarded(c.M, c.D, DT[c.r], "cuda", c.gs)
    gb = Guarded(c.M, c.D, DT[c.gb], "cuda", c.gbs) if c.gb else None
    dgamma, dbeta = Guarded(1, c.D, torch.float32, "cuda"), Guarded(1, c.D, torch.float32, "cuda")
    gsum = Guarded(1, c.D, torch.float32, "cuda") if c.gsum else None
    with hook_off(lib, c.force4 if force4 is None else force4):
        ops.layernorm_bwd(dy.win, x.win, dev(inp["mean"]) if mean is None else mean, dev(inp["rstd"]) if rstd is None else rstd,
                          dev(inp["gamma"]), g_in.win if g_in else None, g_out.win, gb.win if gb else None, dgamma.win,
                          dbeta.win, gsum=gsum.win if gsum else None, gb_scale=dev(inp["col"]), gb_rowscale=dev(inp["row"]),
                          rows_per_group=c.rpg, M=c.M, D=c.D, dy_stride=dy.stride, x_stride=x.stride, g_stride=g_out.stride,
                          gb_stride=gb.stride if gb else None, fold=fold)
        if fold is not None:
            fold.flush()
    torch.cuda.synchronize()
    return dict(g_out=g_out, gb=gb, dgamma=dgamma, dbeta=dbeta, gsum=gsum)


def values(out):
    """(g_out, gb, dgamma, dbeta, gsum) CPU tensors of a run_bwd result, None where the output was not asked for."""
    return tuple(None if out[k] is None else (out[k].cpu() if k in ("g_out", "gb") else out[k].cpu()[0])
                 for k in U.CLASSES_BWD)


def check_bwd(c, inp, out, ref=None, extra=0.0):
    for k, g in out.items():
        assert g is None or g.intact(), f"{c.id}: something outside {k}'s window was written"
    ref = ref or U.bwd_ref(c, inp)
    got = values(out)
    scales = (U.rowmax(ref.g_out), U.rowmax(ref.gb), ref.abs_dgamma, ref.abs_dbeta, ref.abs_gsum)
    for k, t, w, s in zip(U.CLASSES_BWD, got, ref[:5], scales):
        if t is not None:
            U.check(k, c.data, t, w, s, extra)
    return got, ref


def agree(cls, c, a, b, scale):
    """Two launches of different forms on one input: within the class's fp32 bound of each other; two bf16 stores of values
    that close may besides fall on neighbouring bf16 numbers (2^-8 of each value, 2^-7 of one of them with room for the
    other's size)."""
    diff = (a.double() - b.double()).abs()
    if a.dtype == torch.bfloat16:
        diff = ((diff - 2.0 ** -7 * (1 + 2.0 ** -7) * b.double().abs()) / U.BF16_SPREAD).clamp_min(0.0)
    e = U.norm_err(diff, torch.zeros_like(diff), scale)
    assert e <= U.BOUNDS[(cls, c.data)], f"{c.id}: {cls} of the two forms differ by {e:.3e} of the scale"


def fwd_case(ops, lib, c):
    inp = U.fwd_inputs(c)
    return inp, check_fwd(c, inp, run_fwd(ops, lib, c, inp))


def bwd_case(ops, lib, c):
    inp = U.bwd_inputs(c)
    return (inp,) + check_bwd(c, inp, run_bwd(ops, lib, c, inp))


# ------------------------------------------------------------------------------- 1. every form, every dtype ---
@pytest.mark.parametrize("c", U.FWD_FORMS, ids=U.ids(U.FWD_FORMS))
def test_fwd_every_form_and_dtype(ops, lib, c):
    fwd_case(ops, lib, c)


@pytest.mark.parametrize("c", U.BWD_FORMS, ids=U.ids(U.BWD_FORMS))
def test_bwd_every_form_and_dtype(ops, lib, c):
    bwd_case(ops, lib, c)


# ------------------------------------------------------------------------------- 2. the 4-element kernels ---
@pytest.mark.parametrize("c", U.FWD_FOUR, ids=U.ids(U.FWD_FOUR))
def test_fwd_four_element_kernels(ops, lib, c):
    assert c.form[0] == 4
    inp, (y4, m4, r4) = fwd_case(ops, lib, c)
    if c.force4:                                                # the same input on the 8-element form
        y8, m8, r8 = check_fwd(c, inp, run_fwd(ops, lib, c, inp, force4=False))
        wy, wm, wr = U.ref_fwd(inp["x"], inp["gamma"], inp["beta"], c.eps)
        sy, sm = U.fwd_scales(inp["x"], inp["beta"])
        agree("y", c, y4, y8, sy)
        agree("mean", c, m4, m8, sm)
        agree("rstd", c, r4, r8, wr)


@pytest.mark.parametrize("c", U.BWD_FOUR, ids=U.ids(U.BWD_FOUR))
def test_bwd_four_element_kernels(ops, lib, c):
    assert c.form[0] == 4
    inp, got4, ref = bwd_case(ops, lib, c)
    if c.force4:
        got8, _ = check_bwd(c, inp, run_bwd(ops, lib, c, inp, force4=False), ref)
        scales = (U.rowmax(ref.g_out), U.rowmax(ref.gb), ref.abs_dgamma, ref.abs_dbeta, ref.abs_gsum)
        for k, a, b, s in zip(U.CLASSES_BWD, got4, got8, scales):
            if a is not None:
                agree(k, c, a, b, s)


# ------------------------------------------------------------------------------------------- 3. row loops ---
@pytest.mark.parametrize("c", U.FWD_LOOPS, ids=U.ids(U.FWD_LOOPS))
def test_fwd_row_loop(ops, lib, c):
    fwd_case(ops, lib, c)


@pytest.mark.parametrize("c", U.BWD_LOOPS, ids=U.ids(U.BWD_LOOPS))
def test_bwd_row_loop(ops, lib, c):
    bwd_case(ops, lib, c)


# --------------------------------------------------------------------------- 4. strides, guards, aliasing ---
@pytest.mark.parametrize("c", U.FWD_STRIDES, ids=U.ids(U.FWD_STRIDES))
def test_fwd_padded_and_class_token_strides(ops, lib, c):
    fwd_case(ops, lib, c)


@pytest.mark.parametrize("c", U.BWD_STRIDES, ids=U.ids(U.BWD_STRIDES))
def test_bwd_padded_and_class_token_strides(ops, lib, c):
    bwd_case(ops, lib, c)


# ------------------------------------------------------------------------------------- 5. branch scales ---
@pytest.mark.parametrize("c", U.BWD_SCALES, ids=U.ids(U.BWD_SCALES))
def test_bwd_branch_scales(ops, lib, c):
    """gb and gsum carry gb_scale[col] gb_rowscale[row // rpg]; g_out carries neither (check_bwd holds it to the unscaled
    reference); the gb rows of a dropped sample and the columns of a zero LayerScale are exact zeros."""
    inp, got, ref = bwd_case(ops, lib, c)
    gb = got[1].float()
    dropped = inp["row"][torch.arange(c.M) // c.rpg] == 0
    assert dropped.any() and not dropped.all()
    assert (gb[dropped] == 0).all()
    assert (gb[:, inp["col"] == 0] == 0).all()
    assert (gb[~dropped][:, inp["col"] != 0] != 0).any()


# ----------------------------------------------------------------------------------- 6. degenerate rows ---
@pytest.mark.parametrize("c", U.FWD_DEGENERATE, ids=U.ids(U.FWD_DEGENERATE))
def test_fwd_degenerate_rows(ops, lib, c):
    inp, (y, mean, rstd) = fwd_case(ops, lib, c)
    beta = inp["beta"].to(DT[c.ydt])
    if c.special == "const":                                    # x - mean is exactly zero: y is beta, bit for bit
        r = c.M // 2
        assert mean[r].item() == 3.0
        assert torch.equal(y[r], beta)
    if c.special == "gamma0":
        assert torch.equal(y, beta.expand_as(y))


@pytest.mark.parametrize("c", U.BWD_DEGENERATE, ids=U.ids(U.BWD_DEGENERATE))
def test_bwd_degenerate_rows(ops, lib, c):
    """An all-zero dy leaves g_out == g_in exactly and dgamma, dbeta exactly zero; gsum is the column sum of gb, so it is
    exactly zero where there is no g_in and the (scaled) column sum of g_in where there is one."""
    inp, got, ref = bwd_case(ops, lib, c)
    g_out, gb, dgamma, dbeta, gsum = got
    if c.special in ("gamma0", "dy0"):
        want = inp["g_in"] if c.g_in else torch.zeros(c.M, c.D)
        assert torch.equal(g_out.float(), want)
    if c.special == "dy0":
        assert (dgamma == 0).all() and (dbeta == 0).all()
        if not c.g_in:
            assert (gsum == 0).all() and (gb == 0).all()


# --------------------------------------------------------------------------------------- 7. determinism ---
@pytest.mark.parametrize("c", U.DETERMINISM, ids=U.ids(U.DETERMINISM))
def test_bwd_is_deterministic_and_the_deferred_fold_changes_no_bit(ops, lib, c):
    inp = U.bwd_inputs(c)
    first = values(run_bwd(ops, lib, c, inp))
    for k in range(3):
        fold = ops.FoldQueue() if k == 2 else None
        again = values(run_bwd(ops, lib, c, inp, fold=fold))
        for name, a, b in zip(U.CLASSES_BWD, first, again):
            assert (a is None) == (b is None)
            if a is not None:
                assert torch.equal(a, b), f"{c.id}: {name} differs in launch {k + 2}" + (" (deferred fold)" if fold else "")


# ---------------------------------------------------------------------------------------- 8. round trip ---
@pytest.mark.parametrize("c", U.ROUND_TRIP, ids=U.ids(U.ROUND_TRIP))
def test_forward_statistics_into_backward(ops, lib, c):
    """The kernel's own mean / rstd feed the kernel's backward; the reference is float64 from x on.  Bound: the backward
    class's plus the two statistics' (tests/test_layernorm_cpu.py holds the emulated round trip to half of that)."""
    inp = U.bwd_inputs(c)
    f = U.FwdCase(c.id, c.M, c.D, c.r, "f32", c.data, c.eps)
    out = run_fwd(ops, lib, f, dict(x=inp["x"], gamma=inp["gamma"], beta=torch.zeros(c.D)))
    mean, rstd = out["mean"].win[0].contiguous(), out["rstd"].win[0].contiguous()
    _, m64, r64 = U.ref_fwd(inp["x"], inp["gamma"], torch.zeros(c.D), c.eps)
    check_bwd(c, inp, run_bwd(ops, lib, c, inp, mean=mean, rstd=rstd), U.bwd_ref(c, inp, m64, r64),
              extra=U.BOUNDS[("mean", c.data)] + U.BOUNDS[("rstd", c.data)])


# ------------------------------------------------------------------------------------------ 9. refusals ---
def _refused(ops, fn, guards):
    from vit_torch_amd._lib import VitmiError
    with pytest.raises(VitmiError):
        fn()
    torch.cuda.synchronize()
    for g in guards:
        assert g.untouched()


def _fwd_call(ops, M, D, xdt="f32", ydt="f32", xs=None, ys=None, x_mis=0, y_mis=0):
    x = Guarded(M, D, DT[xdt], "cuda", xs, torch.ones(M, D), misalign=x_mis)
    y = Guarded(M, D, DT[ydt], "cuda", ys, misalign=y_mis)
    mean, rstd = Guarded(1, M, torch.float32, "cuda"), Guarded(1, M, torch.float32, "cuda")
    g = torch.ones(D, device="cuda")
    fn = lambda: ops.layernorm_fwd(x.win, g, g, y.win, mean.win, rstd.win, 1e-6, M=M, D=D, x_stride=xs or D, y_stride=ys or D)
    return fn, (y, mean, rstd)


def _bwd_call(ops, M, D, dy="f32", r="f32", gb="f32", st=None, x_mis=0, col_mis=None, short_ws=False):
    st = st or D
    dyt = Guarded(M, D, DT[dy], "cuda", st, torch.ones(M, D))
    x = Guarded(M, D, DT[r], "cuda", st, torch.ones(M, D), misalign=x_mis)
    g_out, gbt = Guarded(M, D, DT[r], "cuda", st), Guarded(M, D, DT[gb], "cuda", st)
    vec = [Guarded(1, D, torch.float32, "cuda") for _ in range(3)]
    ones, stat = torch.ones(D + 4, device="cuda"), torch.ones(M, device="cuda")
    col = None if col_mis is None else ones[col_mis:col_mis + D]
    if not short_ws:
        fn = lambda: ops.layernorm_bwd(dyt.win, x.win, stat, stat, ones[:D], None, g_out.win, gbt.win, vec[0].win, vec[1].win,
                                       gsum=vec[2].win, gb_scale=col, M=M, D=D, dy_stride=st, x_stride=st, g_stride=st,
                                       gb_stride=st)
    else:
        from vit_torch_amd import _lib
        lib = _lib.load()
        need = lib.vitmi_layernorm_bwd_workspace(M, D)
        ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
        ws = ws[(-ws.data_ptr()) % 256:][:need - 1]              # aligned, one byte short
        code = ops.dtype_code
        fn = lambda: _lib.check(lib.vitmi_layernorm_bwd(
            dyt.win.data_ptr(), code(dyt.win), st, x.win.data_ptr(), code(x.win), st, stat.data_ptr(), stat.data_ptr(),
            ones.data_ptr(), None, g_out.win.data_ptr(), code(g_out.win), st, gbt.win.data_ptr(), code(gbt.win), st,
            vec[0].win.data_ptr(), vec[1].win.data_ptr(), vec[2].win.data_ptr(), None, None, 0, M, D, ws.data_ptr(), ws.numel(),
            torch.cuda.current_stream().cuda_stream), "vitmi_layernorm_bwd")
    return fn, [g_out, gbt] + vec


@pytest.mark.parametrize("kw", [dict(D=6), dict(D=2052), dict(D=8, xs=6), dict(D=8, ys=6), dict(D=8, x_mis=1), dict(D=8, y_mis=1)],
                         ids=["D6", "D2052", "x-stride6", "y-stride6", "x-off-by-one", "y-off-by-one"])
def test_fwd_refusals(ops, kw):
    kw = dict(kw)
    D = kw.pop("D")
    if kw.get("xs") == 6 or kw.get("ys") == 6:
        D = 4                                                   # a stride of 6 over rows of 4: no multiple of 4
    fn, guards = _fwd_call(ops, 3, D, **kw)
    _refused(ops, fn, guards)


@pytest.mark.parametrize("kw", [dict(D=6), dict(D=2052), dict(D=4, st=6), dict(D=8, x_mis=1), dict(D=768, short_ws=True),
                                dict(D=100, short_ws=True), dict(D=8, dy="bf16", r="f32", gb="f32"),
                                dict(D=8, dy="bf16", r="bf16", gb="f32"), dict(D=12, dy="bf16", r="f32", gb="f32"),
                                dict(D=8, col_mis=1), dict(D=12, col_mis=1), dict(D=8, col_mis=2)],
                         ids=["D6", "D2052", "stride6", "x-off-by-one", "workspace-short-8", "workspace-short-4", "bf16-f32-f32",
                              "bf16-bf16-f32", "bf16-f32-f32-4", "gb_scale-off-by-one", "gb_scale-off-by-one-4", "gb_scale-off-by-two"])
def test_bwd_refusals(ops, kw):
    kw = dict(kw)
    fn, guards = _bwd_call(ops, 5, kw.pop("D"), **kw)
    _refused(ops, fn, guards)
    assert U.BWD_UNBUILT == (("bf16", "f32", "f32"), ("bf16", "bf16", "f32"))


def test_aligned_gb_scale_is_still_taken(ops, lib):
    """The alignment rule added for gb_scale refuses nothing that ran before: a 16-byte-aligned scale on both forms."""
    for c in (U.BWD_SCALES[0], U.BWD_SCALES[-1]):
        bwd_case(ops, lib, c)
