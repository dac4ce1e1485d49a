"""Float64 references, fp32 host emulations, bounds, guards and the case tables of tests/test_layernorm_*.py.

The kernels are csrc/layernorm.hip: the 8-element form (`ln_fwd8_kernel` / `ln_bwd8_kernel`, a row spread over LPR = 16 / 32 /
64 lanes in NV chunks of 8) and the 4-element form (`ln_fwd_kernel` / `ln_bwd_kernel`, 64 lanes, NV chunks of 4).  A *form*
here is the tuple (E, LPR, NV) with E = 8 or 4; the dispatcher is restated below and tests/test_layernorm_cpu.py checks the
restatement against what the library reports.

`ref_*` are the float64 definitions.  `emu_*` replay the kernels' fp32 arithmetic in torch float32 in the kernels' order
(per-lane chunk sums, the xor butterfly, the per-slot accumulation along the grid-stride walk, the block's slot sum, the
fold) and exist for one purpose: to size the bounds in BOUNDS before any GPU result is seen."""
import zlib
from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch

GUARD = 64                 # sentinel elements before and after a guarded buffer
SENTINEL = -1536.0         # exact in fp32 and in bf16
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
LN_MAX_D = 2048


def f32(x: float) -> float:
    """The value a `float` argument of the C ABI carries (eps)."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------ the dispatcher, restated ---
def ln8_cfg(D):
    for lim, cfg in ((128, (16, 1)), (256, (16, 2)), (384, (16, 3)), (512, (32, 2)), (768, (32, 3)), (1024, (64, 2)),
                     (1536, (64, 3))):
        if D <= lim:
            return cfg
    return (64, 4)


def ln_nv(D):
    return 2 if D <= 512 else 3 if D <= 768 else 4 if D <= 1024 else 8


FORMS8 = ((16, 1), (16, 2), (16, 3), (32, 2), (32, 3), (64, 2), (64, 3), (64, 4))
NVS4 = (2, 3, 4, 8)
BWD8_CAP = {1: 1024, 2: 768, 3: 512, 4: 256}
BWD4_CAP = {2: 1024, 3: 768, 4: 768, 8: 512}
FWD_CAP = 2048


def form_of(D, strides=(), force4=False):
    """(E, LPR, NV) a call takes: the 8-element form needs D % 8 == 0, every stride % 8 == 0 and the hook left on
    (16-byte-aligned pointers besides, which every buffer of these tests has unless a case says otherwise)."""
    if not force4 and D % 8 == 0 and D >= 8 and all(s % 8 == 0 for s in strides):
        return (8,) + ln8_cfg(D)
    return (4, 64, ln_nv(D))


def rpw_of(form):
    return 64 // form[1]


def fwd_blocks(M, form):
    groups = -(-M // rpw_of(form))
    return min(FWD_CAP, -(-groups // 4))


def bwd_blocks(M, form):
    groups = -(-M // rpw_of(form))
    cap = (BWD8_CAP if form[0] == 8 else BWD4_CAP)[form[2]]
    return min(cap, -(-groups // 4))


def workspace_blocks(M, D):
    """Partial rows vitmi_layernorm_bwd_workspace(M, D) reserves: enough for whichever form the call takes."""
    nb = bwd_blocks(M, (4, 64, ln_nv(D)))
    if D % 8 == 0 and D >= 8:
        nb = max(nb, bwd_blocks(M, (8,) + ln8_cfg(D)))
    return nb


def groups_per_wave(M, form, blocks):
    """(fewest, most) row groups a wave of the grid walks."""
    groups = -(-M // rpw_of(form))
    waves = blocks * 4
    return groups // waves, -(-groups // waves)


def loop_rows(form, direction):
    """The smallest M with which every wave walks >= 3 row groups and some walk a 4th: three full sweeps of the capped grid
    and 5 rows (odd, and no multiple of 2 or 4 rows per wave, so the last group is partially live as well)."""
    cap = FWD_CAP if direction == "fwd" else (BWD8_CAP if form[0] == 8 else BWD4_CAP)[form[2]]
    return 3 * 4 * cap * rpw_of(form) + 5


# --------------------------------------------------------------------------------------- float64 references ---
def ref_fwd(x, gamma, beta, eps):
    """float64 (y, mean, rstd); biased variance; eps as the ABI carries it."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(-1)
    d = x - mean[:, None]
    rstd = ((d * d).mean(-1) + f32(eps)) ** -0.5
    return d * rstd[:, None] * gamma + beta, mean, rstd


RefBwd = namedtuple("RefBwd", "g_out gb dgamma dbeta gsum abs_dgamma abs_dbeta abs_gsum")


def ref_bwd(dy, x, mean, rstd, gamma, g_in=None, gb_scale=None, gb_rowscale=None, rpg=1):
    """float64 closed form with mean / rstd as operands, as the kernel has them:
    xh = (x - mean) rstd, a = dy gamma, dx = rstd (a - mean_j a - xh mean_j(a xh)), g_out = g_in + dx,
    gb = g_out gb_scale[col] gb_rowscale[row // rpg]; dgamma = sum_rows dy xh, dbeta = sum_rows dy, gsum = sum_rows gb.
    abs_* are the column sums of the absolute terms, the yardstick of the three sums."""
    dy, x, mean, rstd, gamma = (t.double() for t in (dy, x, mean, rstd, gamma))
    xh = (x - mean[:, None]) * rstd[:, None]
    a = dy * gamma
    dx = rstd[:, None] * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
    g_out = dx if g_in is None else g_in.double() + dx
    gb = g_out
    if gb_scale is not None:
        gb = gb * gb_scale.double()
    if gb_rowscale is not None:
        rows = torch.arange(x.shape[0]) // rpg
        gb = gb * gb_rowscale.double()[rows][:, None]
    t = dy * xh
    return RefBwd(g_out, gb, t.sum(0), dy.sum(0), gb.sum(0), t.abs().sum(0), dy.abs().sum(0), gb.abs().sum(0))


# ------------------------------------------------------------------------------------- fp32 host emulations ---
def _lanes(t, form):
    """[M, D] -> [M, NV, LPR, E]: chunk i of lane l holds columns (i LPR + l) E ...; columns >= D are zeros (adding
    +0.0 is exact, which is what skipping a masked chunk amounts to)."""
    E, L, NV = form
    M, D = t.shape
    assert D <= NV * L * E
    if NV * L * E != D:
        t = torch.nn.functional.pad(t, (0, NV * L * E - D))
    return t.reshape(M, NV, L, E)


def _fma(a, b, c):
    """fl32(a b + c): the product of two fp32 values is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _lane_sum(t4, pairwise=False, times=None):
    """Per-lane sum over the lane's chunks in order; `times`: s = fma(t, times, s) instead of s += t."""
    M, NV, L, E = t4.shape
    s = torch.zeros(M, L, dtype=torch.float32)
    for i in range(NV):
        if pairwise:                                   # ln_fwd_kernel: s += (v0 + v1) + (v2 + v3)
            s = s + ((t4[:, i, :, 0] + t4[:, i, :, 1]) + (t4[:, i, :, 2] + t4[:, i, :, 3]))
        else:
            for j in range(E):
                s = s + t4[:, i, :, j] if times is None else _fma(t4[:, i, :, j], times[:, i, :, j], s)
    return s


def _butterfly(s):
    """v += shfl_xor(v, o) for o = L/2 .. 1; fp32 addition commutes, so every lane ends with the same bits."""
    idx = torch.arange(s.shape[1])
    o = s.shape[1] // 2
    while o:
        s = s + s[:, idx ^ o]
        o //= 2
    return s[:, 0]


def _rsqrt(v):
    return (v.double() ** -0.5).float()                # correctly rounded; the GPU's v_rsq_f32 is within 1 ulp


def _row_sum(t, form, pairwise=False, times=None):
    """Row sum of t (of t * times, each product fused into its addition, where `times` is given) in the form's order."""
    return _butterfly(_lane_sum(_lanes(t, form), pairwise, None if times is None else _lanes(times, form)))


def emu_fwd(x, gamma, beta, eps, form, contract=False):
    """fp32 (y before the store's rounding, mean, rstd) of ln_fwd8_kernel / ln_fwd_kernel on operand values x.  The 8-element
    kernel multiplies the row sums by fl(1/D), the 4-element one divides them by D.  contract: with the multiply-adds the
    compiler may fuse (q += d d; (..) g + b) fused, each rounded once."""
    x, gamma, beta = x.float(), gamma.float(), beta.float()
    D = x.shape[1]
    Df = torch.tensor(float(D), dtype=torch.float32)
    over_d = (lambda s: s / Df) if form[0] == 4 else (lambda s: s * (1.0 / Df))
    mean = over_d(_row_sum(x, form, pairwise=form[0] == 4))
    d = x - mean[:, None]
    var = over_d(_row_sum(d, form, times=d) if contract else _row_sum(d * d, form))
    rstd = _rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    t = d * rstd[:, None]
    return (_fma(t, gamma.expand_as(t), beta.expand_as(t)) if contract else t * gamma + beta), mean, rstd


def _fold(part):
    """fold_rows (csrc/elementwise.hip): 64 row groups stride the partial rows, 4 x 16 of them are summed in order, then
    (t0 + t1) + (t2 + t3)."""
    S, D = part.shape
    R = -(-S // 64)
    if R * 64 != S:
        part = torch.cat([part, torch.zeros(R * 64 - S, D)])
    p = part.reshape(R, 64, D)
    s = torch.zeros(64, D)
    for r in range(R):
        s = s + p[r]
    q = s.reshape(4, 16, D)
    t = torch.zeros(4, D)
    for i in range(16):
        t = t + q[:, i]
    return (t[0] + t[1]) + (t[2] + t[3])


def _walk_sum(terms, form, nb, times=None):
    """Column sum of `terms` [M, D] (of terms * times, fused into the addition, where given) as the backward grid forms it: slot (block, wave, sub-row) adds its rows in the order
    of the grid-stride walk, the block adds its 4 RPW slots (in order for the 8-element form, pairwise for the 4-element
    one), the fold adds the blocks' partial rows."""
    M, D = terms.shape
    rpw = rpw_of(form)
    S = nb * 4 * rpw                                   # row k S + wave rpw + sub belongs to slot (wave, sub)
    K = -(-M // S)
    if K * S != M:
        terms = torch.cat([terms, torch.zeros(K * S - M, D)])
        times = None if times is None else torch.cat([times, torch.zeros(K * S - M, D)])
    t = terms.reshape(K, S, D)
    u = None if times is None else times.reshape(K, S, D)
    acc = torch.zeros(S, D)
    for k in range(K):
        acc = acc + t[k] if u is None else _fma(t[k], u[k], acc)
    blk = acc.reshape(nb, 4 * rpw, D)
    if form[0] == 8:
        a = torch.zeros(nb, D)
        for i in range(4 * rpw):
            a = a + blk[:, i]
    else:
        a = (blk[:, 0] + blk[:, 1]) + (blk[:, 2] + blk[:, 3])
    return _fold(a)


def emu_bwd(dy, x, mean, rstd, gamma, g_in, gb_scale, gb_rowscale, rpg, form, nb=None, contract=False):
    """fp32 (g_out and gb before the stores' rounding, dgamma, dbeta, gsum) of ln_bwd8_kernel / ln_bwd_kernel.  contract: with
    the multiply-adds the compiler may fuse (dg += dy xh; s2 += a xh; (a - c1) - xh c2) fused."""
    dy, x, mean, rstd, gamma = (t.float() for t in (dy, x, mean, rstd, gamma))
    M, D = x.shape
    nb = nb or bwd_blocks(M, form)
    mu, rs = mean[:, None], rstd[:, None]
    inv_d = 1.0 / torch.tensor(float(D), dtype=torch.float32)
    xh = (x - mu) * rs
    a = dy * gamma
    c1 = (_row_sum(a, form) * inv_d)[:, None]
    c2 = ((_row_sum(a, form, times=xh) if contract else _row_sum(a * xh, form)) * inv_d)[:, None]
    o = rs * (_fma(-xh, c2.expand_as(xh), a - c1) if contract else (a - c1) - xh * c2)
    if g_in is not None:
        o = o + g_in.float()
    g_out = o
    if gb_scale is not None:
        o = o * gb_scale.float()
    if gb_rowscale is not None:
        o = o * gb_rowscale.float()[torch.arange(M) // rpg][:, None]
    dgamma = _walk_sum(dy, form, nb, times=xh) if contract else _walk_sum(dy * xh, form, nb)
    return g_out, o, dgamma, _walk_sum(dy, form, nb), _walk_sum(o, form, nb)


# ------------------------------------------------------------------------------------------------ the bounds ---
# B = 4 x the worst error of the fp32 emulation against float64 over every case of the tables below (measured on the host,
# tests/test_layernorm_cpu.py keeps the emulation within B / 2).  Units: y in (1 + |beta_col|); mean in the row's mean |x|;
# rstd relative; g_out / gb in the row's max |g_out| / max |gb|; each column sum in the float64 sum of the absolute terms of
# its column.  Keyed by the data class of the case: residual-stream-like rows (mean 8 sigma, outliers at 50 sigma) lose
# more in x - mean than plain ones, by their construction and not by the kernels' doing.
#                      B            worst emulated, and the case that gave it
BOUNDS = {
    ("y", "plain"): 4.12e-06,      # 1.031e-06  fwdloop-D2048
    ("y", "resid"): 2.8e-05,      # 7.011e-06  fwdloop-D768
    ("mean", "plain"): 4.14e-07,   # 1.034e-07  fwdloop-D64
    ("mean", "resid"): 6.48e-07,   # 1.620e-07  fwd-D1536-f32-bf16
    ("rstd", "plain"): 5e-07,   # 1.250e-07  fwd-D384-bf16-bf16
    ("rstd", "resid"): 1.49e-06,   # 3.727e-07  fwdloop-D768
    ("g_out", "plain"): 9.43e-07,  # 2.357e-07  bwd4-D4-f32-f32-f32
    ("g_out", "resid"): 6.26e-07,  # 1.565e-07  bwd-D96-f32-bf16-bf16
    ("gb", "plain"): 1e-06,     # 2.506e-07  bwdloop-D64-f32-f32-f32
    ("gb", "resid"): 6.26e-07,     # 1.565e-07  bwd-D96-f32-bf16-bf16
    ("dgamma", "plain"): 8.59e-07, # 2.147e-07  bwd-D2048-f32-f32-bf16
    ("dgamma", "resid"): 6.52e-07, # 1.631e-07  bwd-D1544-f32-bf16-f32
    ("dbeta", "plain"): 6.61e-07,  # 1.651e-07  bwd-D768-f32-f32-f32
    ("dbeta", "resid"): 6.36e-07,  # 1.591e-07  bwd-D96-f32-bf16-bf16
    ("gsum", "plain"): 1.43e-06,   # 3.565e-07  bwd-const-D128
    ("gsum", "resid"): 1.39e-05,   # 3.475e-06  bwd4-hook-D768-bf16-f32-bf16
}
CLASSES_FWD = ("y", "mean", "rstd")
CLASSES_BWD = ("g_out", "gb", "dgamma", "dbeta", "gsum")
# Round-to-nearest of a bf16 store: bf16 keeps 8 significant bits, so half a step is 2^-9 of the binade's top and 2^-8 of its
# bottom (16.5 stored for 16.556 is correct rounding, 3.4e-3 off).  2^-8 is the format's unit roundoff; 2^-9 would fail
# correctly rounded stores (tests/test_layernorm_cpu.py shows both).
BF16_U = 2.0 ** -8
BF16_SPREAD = 1.0 + 2.0 ** -8      # what that rounding can add to an error already there

OBSERVED = {}                      # (class, data) -> worst normalised error the checks of this process have seen


def norm_err(got, want, scale, bf16_out=False):
    """max |got - want| / scale in float64 (for a bf16 output: the part of the error its rounding does not explain,
    (|got - want| - 2^-8 |want|) / ((1 + 2^-8) scale)).  Where scale is 0 the value has to be exact: inf otherwise."""
    got, want = got.detach().cpu().double(), want.double()
    scale = scale.double().expand_as(want)
    diff = (got - want).abs()
    if bf16_out:
        diff = ((diff - BF16_U * want.abs()) / BF16_SPREAD).clamp_min(0.0)
    e = torch.where(scale > 0, diff / scale.clamp_min(1e-300), torch.where(diff > 0, float("inf"), 0.0).to(diff.dtype))
    return float(e.max()) if e.numel() else 0.0


def check(cls, data, got, want, scale, extra=0.0):
    """Element-wise: |got - want| <= B scale for an fp32 result, <= 2^-8 |want| + (1 + 2^-8) B scale for a bf16 one."""
    assert torch.isfinite(got.detach().float()).all(), f"{cls}: non-finite values"
    assert tuple(got.shape) == tuple(want.shape), f"{cls}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    e = norm_err(got, want, scale, got.dtype == torch.bfloat16)
    OBSERVED[(cls, data)] = max(OBSERVED.get((cls, data), 0.0), e)
    B = BOUNDS[(cls, data)] + extra
    print(f"ln-err {cls} {data} {e:.3e} bound {B:.3e}")
    assert e <= B, f"{cls} [{data}]: error {e:.3e} of its scale > bound {B:.3e}"
    return e


def fwd_scales(x, beta):
    """(y, mean, rstd-free) scales of a forward: 1 + |beta| per column, the row's mean |x|."""
    return 1.0 + beta.double().abs()[None, :], x.double().abs().mean(-1)


def rowmax(t):
    return t.abs().amax(-1, keepdim=True)


# ------------------------------------------------------------------------------------------------- guards ---
class Guarded:
    """A [rows, D] window of row stride `stride` (>= D) inside one allocation filled with SENTINEL: GUARD sentinels before
    it, the padding of every row, `extra_rows` whole rows and GUARD sentinels after it.  The window starts 16-byte aligned,
    moved `misalign` elements off that on request.  `win` is what a kernel gets; `intact()` says that nothing outside
    rows x D changed."""

    def __init__(self, rows, D, dtype, device, stride=None, values=None, extra_rows=2, misalign=0):
        stride = stride or D
        assert stride >= D
        isz = torch.empty((), dtype=dtype).element_size()
        span = (rows + extra_rows) * stride
        self.full = torch.full((GUARD + 16 // isz + misalign + span + GUARD,), SENTINEL, dtype=dtype, device=device)
        off = GUARD
        while (self.full.data_ptr() + off * isz) % 16:
            off += 1
        off += misalign
        self.off, self.rows, self.D, self.stride = off, rows, D, stride
        self.win = self.full.as_strided((rows, D), (stride, 1), off)
        if values is not None:
            self.win.copy_(values.to(dtype))

    def outside(self):
        f = self.full.detach().clone()
        f.as_strided((self.rows, self.D), (self.stride, 1), self.off).fill_(SENTINEL)
        return f

    def intact(self) -> bool:
        return bool((self.outside() == SENTINEL).all())

    def untouched(self) -> bool:
        """Nothing at all was written (an output that held only sentinels)."""
        return bool((self.full == SENTINEL).all())

    def cpu(self):
        return self.win.detach().cpu().clone()


# ------------------------------------------------------------------------------------------- the case tables ---
@dataclass(frozen=True)
class FwdCase:
    id: str
    M: int
    D: int
    xdt: str = "f32"
    ydt: str = "f32"
    data: str = "plain"
    eps: float = 1e-6
    xs: int = 0                # row strides in elements, 0 = D
    ys: int = 0
    force4: bool = False       # run under vitmi_debug_ln8(0)
    special: str = ""          # "const": row M // 2 is the constant 3.0; "gamma0"

    @property
    def form(self):
        return form_of(self.D, (self.xs or self.D, self.ys or self.D), self.force4)


@dataclass(frozen=True)
class BwdCase:
    id: str
    M: int
    D: int
    dy: str = "f32"
    r: str = "f32"             # x, g_in, g_out
    gb: str = "f32"            # gb_out, "" = absent
    g_in: bool = True
    gsum: bool = True
    data: str = "plain"
    eps: float = 1e-6
    col: bool = False          # gb_scale, with zeros
    rpg: int = 0               # gb_rowscale over groups of rpg rows, with zeros; 0 = absent
    dys: int = 0
    xs: int = 0
    gs: int = 0
    gbs: int = 0
    force4: bool = False
    inplace: bool = False      # g_out is g_in
    special: str = ""          # "const", "gamma0", "dy0"

    @property
    def form(self):
        st = [self.dys or self.D, self.xs or self.D, self.gs or self.D]
        if self.gb:
            st.append(self.gbs or self.D)
        return form_of(self.D, st, self.force4)


FWD_DTYPES = (("f32", "f32"), ("f32", "bf16"), ("bf16", "bf16"), ("bf16", "f32"))
BWD_DTYPES = (("f32", "f32", "f32"), ("bf16", "f32", "bf16"), ("bf16", "bf16", "bf16"), ("f32", "bf16", "f32"),
              ("f32", "f32", "bf16"), ("f32", "bf16", "bf16"))                      # (dy, x/g, gb): every one built
BWD_UNBUILT = (("bf16", "f32", "f32"), ("bf16", "bf16", "f32"))
FORM_D = (96, 192, 384, 512, 768, 1024, 1536, 2048)                                  # one D per 8-element form
EDGE_D = (8, 128, 136, 256, 264, 392, 520, 776, 1032, 1544)                          # the other side of every ln8_cfg step
NAT4_D = (4, 12, 100, 508, 516, 764, 772, 1020, 1028, 2044)                          # D % 8 == 4, both sides of ln_nv's steps
DATA = ("plain", "resid")
EPS = (1e-6, 1e-5)


def _m_form(D):
    rpw = 64 // ln8_cfg(D)[0]
    return 4 * rpw + rpw - 1                           # four full row groups and a partially live fifth


def _bwd_variant(k, dy, r, gb):
    """g_in / gsum / gb_out present or absent, cycled; gb_out can be absent only where its dtype would be dy's."""
    g_in, gsum = k % 2 == 0, k % 3 != 1
    if gb == dy and k % 4 == 3:
        gb = ""
    return dict(dy=dy, r=r, gb=gb, g_in=g_in, gsum=gsum)


def _forms_fwd():
    out, k = [], 0
    for D in FORM_D:
        for xdt, ydt in FWD_DTYPES:
            out.append(FwdCase(f"fwd-D{D}-{xdt}-{ydt}", _m_form(D), D, xdt, ydt, DATA[k % 2], EPS[(k // 2) % 2]))
            k += 1
    for D in EDGE_D:
        xdt, ydt = FWD_DTYPES[k % 4]
        out.append(FwdCase(f"fwd-D{D}-{xdt}-{ydt}", _m_form(D), D, xdt, ydt, DATA[k % 2], EPS[(k // 2) % 2]))
        k += 1
    return out


def _forms_bwd():
    out, k = [], 0
    for D in FORM_D:
        for dy, r, gb in BWD_DTYPES:
            v = _bwd_variant(k, dy, r, gb)
            out.append(BwdCase(f"bwd-D{D}-{dy}-{r}-{gb}", _m_form(D), D, data=DATA[k % 2], eps=EPS[(k // 2) % 2],
                               inplace=v["g_in"] and k % 4 == 0, **v))
            k += 1
    for D in EDGE_D:
        dy, r, gb = BWD_DTYPES[k % 6]
        out.append(BwdCase(f"bwd-D{D}-{dy}-{r}-{gb}", _m_form(D), D, data=DATA[k % 2], eps=EPS[(k // 2) % 2],
                           **_bwd_variant(k, dy, r, gb)))
        k += 1
    return out


def _four_fwd():
    out = []
    for k, D in enumerate(NAT4_D):
        xdt, ydt = FWD_DTYPES[k % 4]
        out.append(FwdCase(f"fwd4-D{D}-{xdt}-{ydt}", 7, D, xdt, ydt, DATA[k % 2], EPS[(k // 2) % 2]))
    out.append(FwdCase("fwd4-stride4mod8-f32", 9, 768, "f32", "f32", xs=772, ys=780))
    out.append(FwdCase("fwd4-stride4mod8-bf16", 9, 768, "bf16", "bf16", "resid", xs=772, ys=780))
    for k, D in enumerate((96, 768, 2048)):
        xdt, ydt = FWD_DTYPES[k % 4]
        out.append(FwdCase(f"fwd4-hook-D{D}-{xdt}-{ydt}", 9, D, xdt, ydt, DATA[k % 2], force4=True))
    return out


def _four_bwd():
    out = []
    for k, D in enumerate(NAT4_D):
        dy, r, gb = BWD_DTYPES[k % 6]
        out.append(BwdCase(f"bwd4-D{D}-{dy}-{r}-{gb}", 7, D, data=DATA[k % 2], eps=EPS[(k // 2) % 2],
                           **_bwd_variant(k, dy, r, gb)))
    out.append(BwdCase("bwd4-stride4mod8-f32", 9, 768, dys=772, xs=780, gs=772, gbs=788, col=True))
    out.append(BwdCase("bwd4-stride4mod8-bf16", 9, 768, "bf16", "bf16", "bf16", data="resid", dys=772, xs=780, gs=772,
                       gbs=788, inplace=True))
    for k, D in enumerate((96, 768, 2048)):
        dy, r, gb = BWD_DTYPES[k % 6]
        out.append(BwdCase(f"bwd4-hook-D{D}-{dy}-{r}-{gb}", 9, D, dy, r, gb, data=DATA[k % 2], force4=True, col=True, rpg=4))
    return out


def _loops_fwd():
    return [FwdCase("fwdloop-D64", loop_rows((8, 16, 1), "fwd"), 64),
            FwdCase("fwdloop-D768", loop_rows((8, 32, 3), "fwd"), 768, "bf16", "bf16", "resid"),
            FwdCase("fwdloop-D2048", loop_rows((8, 64, 4), "fwd"), 2048, "f32", "bf16", eps=1e-5)]


def _loops_bwd():
    out = []
    for k, D in enumerate((64, 192, 384, 512, 768, 1024, 1536, 2048)):
        dy, r, gb = BWD_DTYPES[k % 6]
        out.append(BwdCase(f"bwdloop-D{D}-{dy}-{r}-{gb}", loop_rows((8,) + ln8_cfg(D), "bwd"), D, dy, r, gb,
                           data=DATA[k % 2], eps=EPS[(k // 2) % 2], col=k % 3 == 0, rpg=197 if k % 4 == 1 else 0,
                           inplace=k % 2 == 0))
    for k, D in enumerate((100, 516, 772, 1028)):                                   # one per NV of the 4-element kernel
        dy, r, gb = BWD_DTYPES[(k + 2) % 6]
        out.append(BwdCase(f"bwd4loop-D{D}-{dy}-{r}-{gb}", loop_rows((4, 64, ln_nv(D)), "bwd"), D, dy, r, gb,
                           data=DATA[k % 2], col=k == 1, rpg=50 if k == 2 else 0, inplace=k % 2 == 1))
    return out


def _strides_fwd():
    return [FwdCase("fwd-pad8-f32", 19, 384, xs=392, ys=400),
            FwdCase("fwd-pad8-bf16", 9, 512, "bf16", "bf16", "resid", xs=528, ys=520),
            FwdCase("fwd-cls-D192", 6, 192, xs=5 * 192),
            FwdCase("fwd-cls-D100", 6, 100, "bf16", "f32", xs=5 * 100, ys=104)]


def _strides_bwd():
    return [BwdCase("bwd-pad8-f32", 19, 384, dys=392, xs=400, gs=408, gbs=392),
            BwdCase("bwd-pad8-bf16", 9, 512, "bf16", "bf16", "bf16", data="resid", dys=520, xs=528, gs=520, gbs=536,
                    inplace=True),
            BwdCase("bwd-cls-D192-gin", 6, 192, xs=5 * 192, gs=5 * 192, gb="", inplace=True),
            BwdCase("bwd-cls-D192-nogin", 6, 192, xs=5 * 192, gs=5 * 192, gb="", g_in=False),
            BwdCase("bwd-cls-D100-nogin", 6, 100, "f32", "bf16", "bf16", xs=5 * 100, gs=5 * 100, g_in=False)]


def _scales_bwd():
    out = []
    for D, (dy, r, gb) in ((192, BWD_DTYPES[0]), (768, BWD_DTYPES[1]), (100, BWD_DTYPES[4])):
        for rpg in (1, 7, 9):                          # M = 42: 7 divides it, 9 does not
            out.append(BwdCase(f"bwd-scale-D{D}-rpg{rpg}-{gb}", 42, D, dy, r, gb, col=True, rpg=rpg))
    return out


def _degenerate_fwd():
    return [FwdCase("fwd-M1-D768", 1, 768), FwdCase("fwd-M1-D12", 1, 12, "bf16", "bf16"),
            # a constant row: mean is exact where the row sum times fl(1/D) is (D a power of two) or the kernel divides
            FwdCase("fwd-const-D128", 5, 128, special="const"), FwdCase("fwd-const-D1024", 5, 1024, "f32", "bf16", special="const"),
            FwdCase("fwd-const-D96-4", 5, 96, force4=True, special="const"), FwdCase("fwd-const-D12", 5, 12, special="const"),
            FwdCase("fwd-gamma0-D384", 9, 384, special="gamma0"), FwdCase("fwd-gamma0-D100", 7, 100, "bf16", "f32", special="gamma0")]


def _degenerate_bwd():
    # M = 1 without gsum: there it is gb itself, which the gb class holds element-wise; in units of its own |term| a single
    # element near zero has no bound that means anything
    return [BwdCase("bwd-M1-D768", 1, 768, gsum=False), BwdCase("bwd-M1-D12", 1, 12, "bf16", "bf16", "bf16", gsum=False),
            BwdCase("bwd-const-D128", 5, 128, special="const"), BwdCase("bwd-const-D12", 5, 12, special="const"),
            BwdCase("bwd-gamma0-D384", 9, 384, special="gamma0"), BwdCase("bwd-gamma0-D100", 7, 100, special="gamma0"),
            BwdCase("bwd-dy0-D384-gin", 9, 384, special="dy0", col=True), BwdCase("bwd-dy0-D384-nogin", 9, 384, special="dy0", g_in=False),
            BwdCase("bwd-dy0-D100-bf16", 7, 100, "bf16", "bf16", "bf16", special="dy0", inplace=True)]


FWD_FORMS, BWD_FORMS = _forms_fwd(), _forms_bwd()
FWD_FOUR, BWD_FOUR = _four_fwd(), _four_bwd()
FWD_LOOPS, BWD_LOOPS = _loops_fwd(), _loops_bwd()
FWD_STRIDES, BWD_STRIDES = _strides_fwd(), _strides_bwd()
BWD_SCALES = _scales_bwd()
FWD_DEGENERATE, BWD_DEGENERATE = _degenerate_fwd(), _degenerate_bwd()
ROUND_TRIP = [BwdCase("rt-D768-f32", 37, 768), BwdCase("rt-D768-bf16x", 37, 768, "bf16", "bf16", "bf16"),
              BwdCase("rt-D100-f32", 37, 100), BwdCase("rt-D100-bf16x", 37, 100, "f32", "bf16", "f32")]
DETERMINISM = [BWD_LOOPS[4], BWD_LOOPS[9]]            # D = 768 on the 8-element form, D = 516 on the 4-element one
ALL_FWD = FWD_FORMS + FWD_FOUR + FWD_LOOPS + FWD_STRIDES + FWD_DEGENERATE
ALL_BWD = BWD_FORMS + BWD_FOUR + BWD_LOOPS + BWD_STRIDES + BWD_SCALES + BWD_DEGENERATE + ROUND_TRIP


def ids(cases):
    return [c.id for c in cases]


# -------------------------------------------------------------------------------------------------- inputs ---
def _round(t, dt):
    return t.to(torch.bfloat16).float() if dt == "bf16" else t


def _gen_x(g, M, D, data, special):
    x = torch.randn(M, D, generator=g)
    if data == "plain":
        x = 2 * x + 0.5                                # the existing tests' input
    else:                                              # a late block's residual stream: row mean 8 sigma, outliers at 50 sigma
        x = x + 8.0
        for c in sorted({1 % D, D // 2, D - 2 if D > 2 else 0}):
            x[:, c] += 50.0
    if special == "const":
        x[M // 2] = 3.0                                # every partial sum of the row is a small integer: exact in fp32
    return x


def fwd_inputs(c: FwdCase):
    """fp32 CPU tensors holding the operand values (bf16 operands already rounded): x, gamma, beta."""
    g = torch.Generator("cpu").manual_seed(zlib.crc32(c.id.encode()))
    x = _round(_gen_x(g, c.M, c.D, c.data, c.special), c.xdt)
    gamma = 1 + 0.1 * torch.randn(c.D, generator=g)
    beta = 0.1 * torch.randn(c.D, generator=g)
    if c.special == "gamma0":
        gamma = torch.zeros(c.D)
    return dict(x=x, gamma=gamma, beta=beta)


def bwd_inputs(c: BwdCase):
    """fp32 CPU tensors: dy, x, gamma, g_in, col (gb_scale), row (gb_rowscale), and mean / rstd = the float64 statistics
    of x rounded to fp32, which is what the backward kernel is given."""
    g = torch.Generator("cpu").manual_seed(zlib.crc32(c.id.encode()))
    x = _round(_gen_x(g, c.M, c.D, c.data, c.special), c.r)
    dy = _round(torch.randn(c.M, c.D, generator=g), c.dy)
    gin = _round(torch.randn(c.M, c.D, generator=g), c.r) if c.g_in else None
    gamma = 1 + 0.1 * torch.randn(c.D, generator=g)
    if c.special == "gamma0":
        gamma = torch.zeros(c.D)
    if c.special == "dy0":
        dy = torch.zeros(c.M, c.D)
    col = row = None
    if c.col:
        col = torch.randn(c.D, generator=g)
        col[::5] = 0.0
    if c.rpg:
        n = -(-c.M // c.rpg)
        row = torch.full((n,), 1.25)
        row[torch.rand(n, generator=g) < 0.3] = 0.0
        row[0] = 0.0
        if n > 1:
            row[-1] = 1.25
    _, mean, rstd = ref_fwd(x, gamma, torch.zeros(c.D), c.eps)
    return dict(dy=dy, x=x, gamma=gamma, g_in=gin, col=col, row=row, mean=mean.float(), rstd=rstd.float())


def bwd_ref(c: BwdCase, inp, mean=None, rstd=None):
    return ref_bwd(inp["dy"], inp["x"], inp["mean"] if mean is None else mean, inp["rstd"] if rstd is None else rstd,
                   inp["gamma"], inp["g_in"], inp["col"], inp["row"], c.rpg or 1)


ROW_CHUNK = 8192          # rows of a forward reference held in float64 at a time


def fwd_emu_errors(c: FwdCase, inp):
    """{class: worst normalised error of the emulation against float64} of one forward case."""
    out = dict.fromkeys(CLASSES_FWD, 0.0)
    for r0 in range(0, c.M, ROW_CHUNK):
        x = inp["x"][r0:r0 + ROW_CHUNK]
        wy, wm, wr = ref_fwd(x, inp["gamma"], inp["beta"], c.eps)
        sy, sm = fwd_scales(x, inp["beta"])
        for contract in (False, True):                  # the worse of the two ways the compiler may build it
            y, mean, rstd = emu_fwd(x, inp["gamma"], inp["beta"], c.eps, c.form, contract)
            for k, e in (("y", norm_err(y, wy, sy)), ("mean", norm_err(mean, wm, sm)), ("rstd", norm_err(rstd, wr, wr))):
                out[k] = max(out[k], e)
    return out


def bwd_errors(c: BwdCase, got, ref: RefBwd):
    """{class: normalised error} of (g_out, gb, dgamma, dbeta, gsum) tensors against a RefBwd; bf16 tensors by the bf16 rule."""
    scales = (rowmax(ref.g_out), rowmax(ref.gb), ref.abs_dgamma, ref.abs_dbeta, ref.abs_gsum)
    asked = dict(g_out=True, gb=bool(c.gb), dgamma=True, dbeta=True, gsum=c.gsum)
    return {k: norm_err(t, w, s, t.dtype == torch.bfloat16)
            for k, t, w, s in zip(CLASSES_BWD, got, ref[:5], scales) if t is not None and asked[k]}


def bwd_emu_errors(c: BwdCase, inp, mean=None, rstd=None, ref=None):
    """The same for a backward case, the worse of the un-fused and the fused build; mean / rstd: other statistics than the
    rounded float64 ones (the round trip)."""
    ref = ref or bwd_ref(c, inp)
    out = {}
    for contract in (False, True):
        got = emu_bwd(inp["dy"], inp["x"], inp["mean"] if mean is None else mean, inp["rstd"] if rstd is None else rstd,
                      inp["gamma"], inp["g_in"], inp["col"], inp["row"], c.rpg or 1, c.form, contract=contract)
        for k, e in bwd_errors(c, got, ref).items():
            out[k] = max(out.get(k, 0.0), e)
    return out


def round_trip_emu_errors(c: BwdCase, inp):
    """Emulated forward statistics into the emulated backward, against float64 from x on."""
    worst = {}
    _, m64, r64 = ref_fwd(inp["x"], inp["gamma"], torch.zeros(c.D), c.eps)
    ref = bwd_ref(c, inp, m64, r64)
    for contract in (False, True):
        _, m, r = emu_fwd(inp["x"], inp["gamma"], torch.zeros(c.D), c.eps, form_of(c.D), contract)
        for k, e in bwd_emu_errors(c, inp, m, r, ref).items():
            worst[k] = max(worst.get(k, 0.0), e)
    return worst
