"""What the GEMM tests (tests/test_gemm_cpu.py, tests/test_gemm_gpu.py) compare vitmi_gemm against: the float64 result of
every VITMI_EPI_* as include/vitmi.h defines it, the same mathematics with only the roundings epilogue.h declares, three
seeded input families, strided placement with NaN gaps, and the metrics.  Nothing here touches the library."""
import math
from collections import namedtuple

import torch

EPI_STORE, EPI_BIAS_GELU, EPI_RESIDUAL, EPI_DGELU, EPI_PATCH_POS = 0, 1, 2, 3, 4
EPI_NAMES = {EPI_STORE: "store", EPI_BIAS_GELU: "gelu", EPI_RESIDUAL: "residual", EPI_DGELU: "dgelu", EPI_PATCH_POS: "patchpos"}
F64 = torch.float64
FP32_GRADE = 2e-6          # fp32 sums of exact bf16 products against float64 (the project's bound for them)
COLSUM_ROWS = 128          # rows per colsum_part group

GemmRef = namedtuple("GemmRef", "C C2 colsum")
GemmRef.__doc__ = """C [M,N], C2 [M,N] or None, colsum [ceil(M/128),N] or None; float64."""


def bf16(t):
    """Round to bf16 (nearest even), keeping the dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def f32(t):
    return t.to(torch.float32).to(t.dtype)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def product(A, B, a_kmajor=True, b_kmajor=True):
    """float64 sum_k A(m,k) B(n,k) of the STORED operands: A is [M,K] if a_kmajor else [K,M], B [N,K] / [K,N]."""
    a = A.to(F64) if a_kmajor else A.to(F64).t()
    b = B.to(F64) if b_kmajor else B.to(F64).t()
    return a @ b.t()


def _ident(t):
    return t


def _epilogue(acc, epilogue, rc, rc2, rpre, *, alpha=1.0, C_in=None, bias=None, R=None, gamma=None, rowscale=None,
              rows_per_group=0, aux=None, aux_deriv=False, pos=None, n_tok=0, cls=None, want_c2=False, want_colsum=False):
    """vitmi_gemm's epilogues on a float64 accumulator.  rc / rc2: roundings of the C / C2 stores; rpre: rounding of the
    pre-activation EPI_BIAS_GELU evaluates GELU at (without aux_deriv)."""
    M, N = acc.shape
    d = lambda t: None if t is None else t.to(F64)
    bias, R, gamma, aux, pos, cls, C_in, rowscale = map(d, (bias, R, gamma, aux, pos, cls, C_in, rowscale))
    b = bias if bias is not None else torch.zeros(N, dtype=F64)
    C2 = None
    if epilogue == EPI_STORE:
        v = acc * (alpha if alpha != 0 else 1.0) + b
        if C_in is not None:
            v = v + C_in
    elif epilogue == EPI_BIAS_GELU:
        pre = acc + b
        if aux_deriv:
            v, C2 = gelu64(pre), dgelu64(pre)
        else:
            pre = rpre(pre)
            v, C2 = gelu64(pre), pre
    elif epilogue == EPI_RESIDUAL:
        C2 = acc + b
        v = C2
        if gamma is not None:
            v = v * gamma
        if rowscale is not None:
            rs = rowscale[torch.arange(M) // rows_per_group]
            v = v * rs[:, None]
        v = R + v
    elif epilogue == EPI_DGELU:
        v = acc * (aux if aux_deriv else dgelu64(aux))
    else:
        assert epilogue == EPI_PATCH_POS
        t = torch.arange(M) % n_tok
        p = pos.view(n_tok, N)[t]
        v = acc + b + p
        if cls is not None:
            v = torch.where((t == 0)[:, None], (cls + pos.view(n_tok, N)[0])[None, :].expand(M, N), v)
    colsum = None
    if want_colsum:
        G = (M + COLSUM_ROWS - 1) // COLSUM_ROWS
        pad = torch.zeros((G * COLSUM_ROWS, N), dtype=F64)
        pad[:M] = v
        colsum = pad.view(G, COLSUM_ROWS, N).sum(1)
    return GemmRef(rc(v), rc2(C2) if (C2 is not None and want_c2) else None, colsum)


def reference(A, B, *, a_kmajor=True, b_kmajor=True, epilogue=EPI_STORE, acc=None, **k):
    """float64 vitmi_gemm: no rounding anywhere.  `acc`, if given, is product(A, B, ...) computed before (cases that
    run several epilogues on one product share it).  Keywords: alpha, C_in (the C that `accumulate` adds to), bias, R,
    gamma, rowscale, rows_per_group, aux, aux_deriv, pos, n_tok, cls, want_c2, want_colsum."""
    if acc is None:
        acc = product(A, B, a_kmajor, b_kmajor)
    return _epilogue(acc, epilogue, _ident, _ident, _ident, **k)


def emulated(A, B, *, c_bf16, in_bf16=True, rounding=True, a_kmajor=True, b_kmajor=True, epilogue=EPI_STORE, acc=None, **k):
    """The same mathematics with only the roundings epilogue.h declares: C and C2 are rounded to their dtype at the
    store (C2: C's dtype for EPI_BIAS_GELU, the operand dtype for EPI_RESIDUAL); EPI_BIAS_GELU without aux_deriv
    evaluates GELU at the bf16-rounded pre-activation when C is bf16.  colsum_part sums the unrounded values.
    rounding=False: equal to `reference`."""
    if acc is None:
        acc = product(A, B, a_kmajor, b_kmajor)
    if not rounding:
        return _epilogue(acc, epilogue, _ident, _ident, _ident, **k)
    rc = bf16 if c_bf16 else f32
    rc2 = (bf16 if in_bf16 else f32) if epilogue == EPI_RESIDUAL else rc
    rpre = bf16 if c_bf16 else _ident
    return _epilogue(acc, epilogue, rc, rc2, rpre, **k)


# ------------------------------------------------------------------------------------------------ inputs ---
def _gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def row_scales(n, period, shift):
    """2^((i mod period) - shift), float64 (exact in bf16)."""
    return torch.pow(2.0, ((torch.arange(n) % period) - shift).to(F64))


def make_inputs(family, M, N, K, epilogue, seed, *, in_bf16=True, side_bf16=False, n_tok=0, rows_per_group=0, big_rows=1.0):
    """One problem's inputs as float64 CPU tensors holding values exact in the dtype they will be stored in:
    a [M,K], b [N,K] (logical, k-major), bias [N], R [M,N], C_in [M,N], gamma [N], rowscale [groups], aux [M,N],
    pos [n_tok*N], cls [N], and `norm` [M,N]: what the result is divided by before errors are measured (ones except for
    `scaled`).  A caller passes on what its epilogue uses.  side_bf16: R is stored in bf16.  big_rows: `integer` only,
    factor on the rows of a whose rowscale is 0 (the dropped branch may be large).
      normal   unit-normal a, 0.2 x unit-normal b (bf16-rounded if in_bf16); bias, pos, cls, R, C_in normal at the
               product's standard deviation 0.2 sqrt(K), so that every term of an epilogue weighs the same and no row
               (a dropped DropPath group, a CLS row) is much smaller than the rest; gamma 1 + 0.3 normal; rowscale 0 or 1 / 0.75;
               aux = gelu'(|unit normal|), what aux_is_derivative stores for a non-negative pre-activation
      scaled   normal with row m of a times 2^((m mod 7) - 3), row n of b times 2^((n mod 5) - 2); R and C_in scaled by
               both; bias / pos / cls, which cannot carry a per-row factor, by b's factor / 8: their weight in the normalised
               result runs from 1 (rows scaled 2^-3) down to 2^-6; norm = the product of the two scales
      integer  a, b in {-1, 0, 1} with P(non-zero) = 1/4; bias, R, C_in, pos, cls integers in -3..3; gamma in
               {+-1, +-2, 4}; rowscale in {0, 1, 2}; aux in -2..2 (for aux_deriv)"""
    g = _gen(seed)
    rin = bf16 if in_bf16 else f32
    rside = bf16 if side_bf16 else f32
    G = (M + rows_per_group - 1) // rows_per_group if rows_per_group else 0
    x = {}
    if family == "integer":
        tern = lambda shape: ((torch.rand(shape, generator=g) < 0.25).to(F64) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(F64))
        small = lambda shape: torch.randint(-3, 4, shape, generator=g).to(F64)
        x["a"], x["b"] = tern((M, K)), tern((N, K))
        x["bias"], x["R"], x["C_in"], x["cls"] = small((N,)), small((M, N)), small((M, N)), small((N,))
        x["gamma"] = torch.tensor([1.0, -1.0, 2.0, -2.0, 4.0], dtype=F64)[torch.randint(0, 5, (N,), generator=g)]
        x["aux"] = torch.randint(-2, 3, (M, N), generator=g).to(F64)
        x["pos"] = small((max(n_tok, 1) * N,))
        if G:
            x["rowscale"] = torch.randint(0, 3, (G,), generator=g).to(F64)
            x["rowscale"][0] = 0.0                       # always at least one dropped group
            if big_rows != 1.0:
                drop = x["rowscale"][torch.arange(M) // rows_per_group] == 0
                x["a"][drop] *= big_rows
        x["norm"] = torch.ones((M, N), dtype=F64)
        return x
    assert family in ("normal", "scaled")
    rn = lambda shape: torch.randn(shape, generator=g).to(F64)
    x["a"], x["b"] = rin(rn((M, K))), rin(rn((N, K)) * 0.2)
    s = 0.2 * math.sqrt(K)                               # the product's own scale: every term of an epilogue then weighs the same
    x["bias"], x["cls"], x["pos"] = f32(s * rn((N,))), f32(s * rn((N,))), f32(s * rn((max(n_tok, 1) * N,)))
    x["R"], x["C_in"] = rside(s * rn((M, N))), f32(s * rn((M, N)))
    x["gamma"] = f32(1.0 + 0.3 * rn((N,)))
    # what aux_is_derivative stores, on the non-negative half: gelu'(|z|) in [0.5, 1.13].  A factor that comes near zero
    # would make the output's density peak at zero, and the rounding band (a share of 1 / |value|) several times wider;
    # signs and zeros of AUX are the `integer` family's, the zero crossing of gelu' section 3.3's
    x["aux"] = rin(dgelu64(rn((M, N)).abs()))
    if G:
        keep = (torch.rand((G,), generator=g) < 0.75).to(F64)
        x["rowscale"] = f32(keep / 0.75)
    x["norm"] = torch.ones((M, N), dtype=F64)
    if family == "scaled":
        sa, sb = row_scales(M, 7, 3), row_scales(N, 5, 2)
        x["a"] = x["a"] * sa[:, None]
        x["b"] = x["b"] * sb[:, None]
        x["norm"] = sa[:, None] * sb[None, :]
        x["R"], x["C_in"] = x["R"] * x["norm"], x["C_in"] * x["norm"]
        x["bias"], x["cls"] = x["bias"] * sb / 8, x["cls"] * sb / 8
        x["pos"] = (x["pos"].view(-1, N) * sb / 8).reshape(-1)
    return x


def integer_conditions(want, bf16_out):
    """The `integer` family's conditions on a reference output (None = met, else the reason): max |want| <= 256 for a
    bf16 output, < 2^24 otherwise, and every value exactly representable in the output dtype."""
    m = want.abs().max().item()
    if bf16_out and m > 256:
        return f"max |want| = {m} > 256 for a bf16 output"
    if not bf16_out and m >= 2 ** 24:
        return f"max |want| = {m} >= 2^24"
    if not torch.equal((bf16 if bf16_out else f32)(want), want):
        return "a reference value is not exact in the output dtype"
    return None


# --------------------------------------------------------------------------------------------- placement ---
def place(x, extra, dtype, device="cpu", border=2, rows_alloc=None, surplus=float("nan")):
    """x [rows, cols] at leading dimension cols + extra inside a NaN-filled buffer with `border` rows above and below
    (rows_alloc > rows: that many rows belong to the matrix; the surplus rows' columns hold `surplus`).  Returns (buffer,
    view of the rows x cols matrix): over-reads of an input hit NaN, stores outside an output destroy NaN canaries."""
    rows, cols = x.shape
    ra = rows_alloc or rows
    buf = torch.full((ra + 2 * border, cols + extra), float("nan"), dtype=dtype, device=device)
    view = buf[border:border + rows, :cols]
    view.copy_(x.to(dtype))
    if ra > rows:
        buf[border + rows:border + ra, :cols] = surplus
    return buf, view


def canaries_intact(buf, rows, cols, border=2, rows_alloc=None):
    """True if everything of `buf` outside its rows_alloc x cols matrix is still NaN."""
    ra = rows_alloc or rows
    b = buf.float()
    return bool(torch.isnan(b[:border]).all() and torch.isnan(b[border + ra:]).all() and torch.isnan(b[:, cols:]).all())


# ----------------------------------------------------------------------------------------------- metrics ---
def rel(got, want, norm=None):
    """max |got - want| / max |want| in float64; with `norm` both sides are divided by it first (the `scaled` family:
    every element then has the same expected magnitude)."""
    g, w = got.to(F64), want.to(F64)
    if norm is not None:
        g, w = g / norm, w / norm
    d = w.abs().max().item()
    return (g - w).abs().max().item() / (d if d > 0 else 1.0)


def rne_bf16(x):
    """Round-to-nearest-even of float64 values to bf16 (8 significant bits, exponents down to the denormals of 2^-133),
    returned as float64; no double rounding through fp32."""
    _, e = torch.frexp(x)
    ulp = torch.pow(2.0, (e.clamp(min=-125) - 8).to(F64))
    return torch.round(x / ulp) * ulp


def rounding_check(got, want64, delta, norm=None):
    """Is the bf16 tensor `got` the round-to-nearest-even bf16 of `want64`, allowing an error `delta` (absolute) in the
    value that was rounded?  An element passes iff RNE(want - delta) <= got <= RNE(want + delta).  Where want lies further
    than delta from every bf16 rounding boundary that is got == RNE(want) and nothing else; where a boundary is within delta
    the bf16 value on its other side passes too; a distance of two ulps or a mismatch outside that band fails.  (Where
    delta exceeds an ulp — elements near zero — the same rule accepts every bf16 value delta can reach.)
    Returns (number of failing elements, share of elements whose band holds more than one bf16 value — from the reference
    alone —, worst |got - want|)."""
    g, w = got.to(F64), want64.to(F64)
    if norm is not None:
        g, w = g / norm, w / norm
    lo, hi = rne_bf16(w - delta), rne_bf16(w + delta)
    bad = ~((g >= lo) & (g <= hi))          # NaN fails
    share = (lo != hi).double().mean().item()
    return int(bad.sum().item()), share, (g - w).abs().max().item()


def band_share(want64, delta, norm=None):
    w = want64 if norm is None else want64 / norm
    return (rne_bf16(w - delta) != rne_bf16(w + delta)).double().mean().item()


# ------------------------------------------------------------------------ the tile kernels' GELU on the CPU ---
def finite_bf16_line():
    """Every finite bf16 value once, as float32 [65280], in bit-pattern order."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    keep = ((bits >> 7) & 0xFF) != 0xFF
    return (bits[keep] << 16).view(torch.float32).clone()


def gelu_grid():
    """The line laid out [256, 256] (zero-padded): entry [k, n] is the argument of output element (m = k, n)."""
    v = finite_bf16_line()
    g = torch.zeros(256 * 256, dtype=torch.float32)
    g[:v.numel()] = v
    return g.view(256, 256)


def tile_gelu_f32(x):
    """gemm_tile.h's gelu_tail2 / gelu2 / dgelu2 in float32 torch arithmetic (separate multiplies and adds where the
    kernel fuses them): returns (gelu, gelu')."""
    x = x.to(torch.float32)
    one = torch.tensor(1.0, dtype=torch.float32)
    e = torch.exp2((x * x) * -0.72134752044)
    t = one / (x.abs() * 0.2316419 + 1.0)
    p = t * 0.5307027145 + -0.7265760135
    p = p * t + 0.7107068705
    p = p * t + -0.142248368
    p = p * t + 0.127414796
    h = (p * t) * e
    gl = -x.abs() * h + x.clamp(min=0.0)
    d = torch.copysign(0.5 - h, x)
    dg = (x * e) * 0.39894228040143267794 + (d + 0.5)
    return gl, dg


SMALL_LO, SMALL_HI = 2.0 ** -100, 1.0      # the arguments whose GELU is also checked relative to |x|


def tile_gelu_errors():
    """Worst error of tile_gelu_f32 against float64 over every finite bf16 argument: (gelu, gelu') absolute, and gelu's
    error relative to |x| over SMALL_LO <= |x| <= SMALL_HI (where gelu(x) ~ x / 2 and an absolute bound says little)."""
    x = finite_bf16_line()
    gl, dg = tile_gelu_f32(x)
    x64 = x.to(F64)
    eg = (gl.to(F64) - gelu64(x64)).abs()
    small = (x64.abs() >= SMALL_LO) & (x64.abs() <= SMALL_HI)
    return eg.max().item(), (dg.to(F64) - dgelu64(x64)).abs().max().item(), (eg[small] / x64[small].abs()).max().item()


def torch_gelu_f32_errors():
    """Worst absolute error of float32 F.gelu / its autograd derivative against float64 on the same line, over the
    arguments at which torch's own result is finite (its F.gelu overflows to inf at the top few bf16 values, where
    gelu(x) = x is representable)."""
    x = finite_bf16_line().clone().requires_grad_(True)
    y = torch.nn.functional.gelu(x)
    y.sum().backward()
    x64 = x.detach().to(F64)
    eg = (y.detach().to(F64) - gelu64(x64)).abs()
    ed = (x.grad.to(F64) - dgelu64(x64)).abs()
    return eg[torch.isfinite(eg)].max().item(), ed[torch.isfinite(ed)].max().item()


# --------------------------------------------------------------------------------------------- the cases ---
LAYOUTS = {"nt": (True, True), "nn": (True, False), "tn": (False, False), "tt": (False, True)}
RPG, NTOK = 50, 7          # rows per rowscale group / tokens per image of EPI_PATCH_POS: neither divides a tile


def rpg(M):
    """Rows per rowscale group at M rows: RPG, or a third of a short matrix (at least three groups: the first one is
    always dropped, and a case whose every row is dropped would not see gamma or the branch at all)."""
    return min(RPG, max(1, M // 3))
ALL_EPIS = (EPI_STORE, EPI_BIAS_GELU, EPI_RESIDUAL, EPI_DGELU, EPI_PATCH_POS)
LINEAR_EPIS = (EPI_STORE, EPI_RESIDUAL, EPI_DGELU, EPI_PATCH_POS)
TAIL_CUS = 256
# FastPlanKind (gemm_tile.h), as vitmi_debug_gemm_plan reports it; -1 = the call does not take the tile kernels
PLAN_KINDS = {"WHOLE": 0, "SPLITK": 1, "TAIL_FINISHER": 2, "TAIL_FIXUP": 3, "TILE2_WHOLE": 4, "TILE2_SPLITK": 5}
_PIPE_KS = (64, 128, 192, 256, 320)


def tile_combo_built(layout, epi, c_bf16):
    """Which (layout, epilogue, C dtype) the tile kernels instantiate (gemm_tile.h dispatch_combo)."""
    if epi == EPI_STORE:
        return layout in ("nt", "nn", "tn")
    if epi == EPI_BIAS_GELU:
        return layout == "nt" and c_bf16
    if epi == EPI_DGELU:
        return layout == "nn" and c_bf16
    return layout == "nt"


def _p(kind, shapes, *, in_bf16=True, layouts=("nt", "nn", "tn"), epis=ALL_EPIS, shapes32=(), c_f32_only=False, **extra):
    d = dict(kind=kind, shapes=tuple(shapes), in_bf16=in_bf16, layouts=layouts, epis=epis, shapes32=tuple(shapes32),
             c_f32_only=c_f32_only)
    d.update(extra)
    return d


_GEN_SHAPES = ((130, 75, 40), (5, 384, 96), (333, 129, 65))
_PIPE_SHAPES = tuple((512, 256, k) for k in _PIPE_KS) + tuple((256, 768, k) for k in _PIPE_KS)
# path -> what runs on it.  kind: "generic" (impl = GENERIC), "skinny" (AUTO, fp32), "tile" (the tile kernels; the case
# asserts vitmi_gemm_uses_fast).  shapes: section 3.1 (M, N, K[, layout]); shapes32: section 3.2.
PATHS = {
    "generic.bf16": _p("generic", _GEN_SHAPES, layouts=("nt", "nn", "tn", "tt"), shapes32=((333, 129, 65),)),
    "generic.fp32": _p("generic", _GEN_SHAPES, in_bf16=False, layouts=("nt", "nn", "tn", "tt"), shapes32=((333, 129, 65),)),
    "skinny": _p("skinny", ((37, 16, 100, "nt"), (5, 1, 64, "nt"), (37, 100, 16, "nn"), (16, 100, 37, "tn"), (16, 100, 8192, "tn")),
                 in_bf16=False, shapes32=((37, 16, 100, "nt"), (37, 100, 16, "nn"), (16, 100, 8192, "tn"))),
    # (section 3.2 on the 21 M-element walk: the plain store only; its epilogues are the pipe paths')
    "t256.walk": _p("tile", ((256 * 40, 256 * 8, 64),), bands=(-1, 2, 5), shapes32=((256 * 40, 256 * 8, 64, "nt"),), epis32=(EPI_STORE,)),
    # (only the fp32 residual can be folded through LDS)
    "t256.rfold": _p("tile", ((512, 256, 640), (256, 256, 1024)), epis=(EPI_STORE, EPI_RESIDUAL), rfolds=(1, 0),
                     c_f32_only=True, layouts=("nt",), shapes32=((512, 768, 3072),)),
    "t256.splitk": _p("tile", ((256, 256, 1088), (512, 256, 6464)), epis=(EPI_STORE,), c_f32_only=True, needs_ws=True,
                      shapes32=((512, 256, 6464), (256, 256, 12608, "tn"))),
    "t256.tail": _p("tile", ((256 * (TAIL_CUS // 3 + 21), 768, 384),), layouts=("nt", "nn"), epis=(EPI_STORE, EPI_RESIDUAL),
                    fixups=(0, 1), needs_ws=True, no=("acc",), shapes32=((256 * (TAIL_CUS // 3 + 21), 768, 384, "nt"),),
                    epis32=(EPI_RESIDUAL,)),
    "t256.padded": _p("tile", ((300, 256, 64), (640, 768, 192)), layouts=("nt", "nn"), padded=True, no=("acc", "rowscale"),
                      shapes32=((640, 768, 192),)),
    "t128": _p("tile", ((264, 8, 64), (130, 72, 96), (392, 96, 96), (1000, 200, 160), (96, 160, 960, "tn"), (130, 72, 1056)),
               shapes32=((1000, 200, 160), (392, 96, 96), (96, 160, 960, "tn"))),
}
for _pm in range(4):
    for _persist in (1, 0):
        PATHS[f"t256.p{_pm}.{'persist' if _persist else 'onetile'}"] = _p(
            "tile", _PIPE_SHAPES, pipe=_pm, persist=_persist, shapes32=((512, 768, 3072), (256, 768, 192)) if _persist else ())


def option_sets(epi, c_bf16, tile):
    """The option combinations of section 3.1 for one epilogue, richest first.  bias / gamma / rowscale / C2 / cls:
    that side input is passed; alpha: 0.5; acc: accumulate; big: the rows of A whose rowscale is 0 are multiplied by 64;
    deriv: aux_is_derivative; colsum: colsum_part (tile kernels only)."""
    if epi == EPI_STORE:
        s = [("bias", "alpha"), (), ("bias",), ("alpha",)]
        return s if c_bf16 else [("bias", "alpha", "acc")] + s
    if epi == EPI_BIAS_GELU:
        return [("bias", "C2"), ("C2",)]
    if epi == EPI_RESIDUAL:
        return [("bias", "gamma", "rowscale", "C2"), (), ("bias", "C2"), ("gamma", "rowscale", "big")]
    if epi == EPI_DGELU:
        return ([("deriv", "colsum")] if tile else []) + [("deriv",)]
    return [("bias", "cls"), ("cls",), ("bias",), ()]


BIG_ELEMS = 1 << 21        # outputs beyond this many elements run one option set per epilogue


def cases(path, section):
    """(M, N, K, layout, epi, c_bf16, opts) of `path` for section "3.1" (exact) or "3.2" (accuracy: linear epilogues,
    deriv always on for EPI_DGELU)."""
    P = PATHS[path]
    tile = P["kind"] == "tile"
    for shp in (P["shapes"] if section == "3.1" else P["shapes32"]):
        M, N, K = shp[:3]
        for layout in ((shp[3],) if len(shp) > 3 else P["layouts"]):
            if tile and not LAYOUTS[layout][0] and M % 8:
                continue                                   # a k-minor A needs M % 8 == 0 on the tile kernels
            if tile and P.get("padded") and not LAYOUTS[layout][0]:
                continue
            for epi in P["epis"]:
                if section == "3.2" and (epi not in LINEAR_EPIS or epi not in P.get("epis32", ALL_EPIS)):
                    continue
                for c_bf16 in ((False,) if P["c_f32_only"] else (True, False)):
                    if not P["in_bf16"] and c_bf16:
                        continue                           # fp32 operands: fp32 outputs (the parity mode)
                    if tile and not tile_combo_built(layout, epi, c_bf16):
                        continue
                    sets = [o for o in option_sets(epi, c_bf16, tile) if not set(o) & set(P.get("no", ()))]
                    if section == "3.2":
                        sets = [tuple(x for x in sets[0] if x != "alpha")]
                    elif M * N > BIG_ELEMS or P.get("persist") == 0:
                        sets = sets[:1]                    # (the one-tile launch shares its epilogues with the persistent one)
                    for o in sets:
                        yield M, N, K, layout, epi, c_bf16, o


def big_factor(opts, K):
    return 64.0 if "big" in opts else 1.0


def ref_kwargs(x, epi, opts):
    """The reference()/emulated() keywords of one case from make_inputs' dict."""
    k = {}
    if "bias" in opts:
        k["bias"] = x["bias"]
    if epi == EPI_STORE:
        k["alpha"] = 0.5 if "alpha" in opts else 1.0
        if "acc" in opts:
            k["C_in"] = x["C_in"]
    elif epi == EPI_BIAS_GELU:
        k["want_c2"] = "C2" in opts
        k["aux_deriv"] = "deriv" in opts
    elif epi == EPI_RESIDUAL:
        k["R"] = x["R"]
        k["want_c2"] = "C2" in opts
        if "gamma" in opts:
            k["gamma"] = x["gamma"]
        if "rowscale" in opts:
            k["rowscale"], k["rows_per_group"] = x["rowscale"], rpg(x["a"].shape[0])
    elif epi == EPI_DGELU:
        k["aux"], k["aux_deriv"] = x["aux"], "deriv" in opts
        k["want_colsum"] = "colsum" in opts
    else:
        k["pos"], k["n_tok"] = x["pos"], NTOK
        if "cls" in opts:
            k["cls"] = x["cls"]
    return k
