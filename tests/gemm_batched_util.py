"""What the batched-GEMM tests (tests/test_gemm_batched_cpu.py, tests/test_gemm_batched_gpu.py) run vitmi_gemm with
batch > 1 on: the case table, the placement of a batch of problems in NaN-filled storages at two-level batch strides, a
Python mirror of the dispatch (gemm_small_form + small_lds_ok + choose_path, gemm.hip / gemm_small.hip) and of the
workgroups-per-problem rule (gemm_small_parts), and the float64 reference.  Inputs, metrics and bounds are gemm_util's.
Nothing here launches anything; `descriptor` only fills the ctypes struct.

A case is one batched call: `batch = outer * inner` problems of M x N x K in one layout (gemm_util.LAYOUTS).  Problem
(zo, zi) of an operand starts at element off + zo * bs[0] + zi * bs[1] of its storage and has the leading dimension ld.
  plain geometry   every operand in a storage of its own, ld = ru8(row) + 8 (so the columns row .. ld of every row, the pad
                   columns K .. ru8(K) / M .. ru8(M) of an S-type operand among them, are NaN), gaps of 16 / 24 elements
                   between the problems of the inner / outer level, 64 elements before the first and after the last
  th geometries    the six products of ops.th_three_call_fwd / _bwd on their own views: q, k, v inside one [B, T, 3, H, hd]
                   storage, the scores / probabilities [B, H, T, ru8(T)], dO and O [B, T, H, hd], dqkv [B, T, 3, H, hd];
                   what no operand of the call covers (the third of qkv the call does not read, the pad columns T .. ru8(T))
                   is NaN
An output storage is NaN-filled: an element not written stays NaN, and a store outside a problem's M x N window, into the
neighbouring problem's pad columns included, destroys a canary."""
import functools
import zlib
from types import SimpleNamespace

import torch

import gemm_util as U
from gemm_util import F64

PATH_FAST, PATH_SMALL, PATH_SKINNY, PATH_GENERIC = 0, 1, 2, 3          # GemmPath (gemm.hip)
PATH_NAMES = {PATH_FAST: "tile", PATH_SMALL: "small", PATH_SKINNY: "skinny", PATH_GENERIC: "generic"}
GEMM_AUTO, GEMM_GENERIC = 0, 1
F32_CODE, BF16_CODE = 0, 1
SB_MAXN, SB_MAXK, SB_CHUNK, LDS_CAP = 64, 256, 64, 96 * 1024           # gemm_small.hip
MAX_BATCH = 65535                                                      # build_args
DEVICE_CUS = 256                                                       # vitmi_cu_count() of an MI355X, and without a device
FRONT = TAIL = 64                                                      # NaN elements before / after every storage's content
TH = (2, 197, 3, 48)                                                   # (B, T, H, hd) of the th geometries


def ru(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ cases ---
CASES = {}


def _c(name, layout, M, N, K, batch=(2, 3), *, path="small", form=None, parts=None, why=None, group=None, exact_only=False,
       in_bf16=True, c_bf16=True, impl=GEMM_AUTO, small_hook=None, parts_hook=0, geo="plain", lda=None, ldc=None,
       a_shift=0, c_shift=0, a_bs1=None, alpha=1.0, at=()):
    """path / form / parts: what the case is named after (parts None: whatever the heuristic gives); why: the condition
    that sends a fallback case to the generic kernel (small_form's name for it); small_hook / parts_hook: the values of
    vitmi_debug_gemm_small / _small_parts; lda / ldc / a_bs1: instead of the plain geometry's; a_shift / c_shift: elements
    added to the operand's offset; alpha: of the accuracy section; at: the limits of the dispatch this case sits ON."""
    assert name not in CASES
    if path == "small":
        form = {"nt": 0, "nn": 1, "tn": 2}[layout]
    CASES[name] = SimpleNamespace(name=name, layout=layout, M=M, N=N, K=K, outer=batch[0], inner=batch[1], path=path, form=form,
                                  parts=parts, why=why, group=group or name.split(".")[0], exact_only=exact_only,
                                  in_bf16=in_bf16, c_bf16=c_bf16, impl=impl, small_hook=small_hook, parts_hook=parts_hook,
                                  geo=geo, lda=lda, ldc=ldc, a_shift=a_shift, c_shift=c_shift, a_bs1=a_bs1, alpha=alpha, at=at)


B35 = (5, 7)
TH_ALPHA = float(torch.tensor(TH[3] ** -0.5, dtype=torch.float32))
_T, _HD = TH[1], TH[3]
# --- small.form0 (nt): K = head dim
for _k in (8, 32, 40, 48, 64):
    _c(f"f0.K{_k}", "nt", 65, 65, _k, at=("form0 K > 64",) if _k == 64 else ())
for _m in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129):
    _c(f"f0.M{_m}", "nt", _m, 40, 48, B35 if _m <= 17 else (2, 3))
for _n in (9, 17, 197, 672):
    _c(f"f0.N{_n}", "nt", 33, _n, 48, at=("LDS cap",) if _n == 672 else ())
_c("f0.N8", "nt", 33, 8, 48, exact_only=True)
_c("f0.577", "nt", 577, 577, 64, (2, 2))
_c("f0.scores", "nt", _T, _T, _HD, TH[::2], geo="scores", alpha=TH_ALPHA)
_c("f0.dpm", "nt", _T, _T, _HD, TH[::2], geo="dpm")
_c("f0.c_off1", "nt", 33, 40, 48, c_shift=1)                            # store_tile_T's scalar store: C not 8-byte aligned
_c("f0.ldc_n2", "nt", 33, 40, 48, ldc=42)                               # ... and ldc % 4 != 0
# --- small.form1 (nn): K = tokens, N = head dim
_c("f1.K1", "nn", 33, 48, 1, B35, exact_only=True)
for _k in (7, 8, 31, 32, 33, 63, 64, 65, 197, 255, 256):
    _c(f"f1.K{_k}", "nn", 33, 48, _k, B35, at=("K > 256",) if _k == 256 else ())
for _n in (8, 64):
    _c(f"f1.N{_n}", "nn", 33, _n, 70, at=("N > 64",) if _n == 64 else ())
_c("f1.M1", "nn", 1, 48, 70, B35, exact_only=True)
for _m in (17, 129, 300):
    _c(f"f1.M{_m}", "nn", _m, 48, 70)
_c("f1.lda_exact", "nn", 33, 48, 197, lda=200)                          # lda = ru8(K): the last 16-B piece ends the row
_c("f1.pv", "nn", _T, _HD, _T, TH[::2], geo="pv")
_c("f1.dq", "nn", _T, _HD, _T, TH[::2], geo="dq", alpha=TH_ALPHA)
# --- small.form2 (tn): the chunk (64) and prefetch edges in K, the row tiles per wave in M
_c("f2.K1", "tn", 33, 48, 1, exact_only=True)
for _k in (31, 33, 63, 64, 65, 127, 128, 129, 197, 256):
    _c(f"f2.K{_k}", "tn", 33, 48, _k, at=("K > 256",) if _k == 256 else ())
_c("f2.M1", "tn", 1, 48, 70, B35, exact_only=True)
for _m in (16, 17, 64, 65, 197, 255, 256):
    _c(f"f2.M{_m}", "tn", _m, 48, 70, B35 if _m <= 65 else (2, 3), at=("form2 M > 256",) if _m == 256 else ())
for _n in (8, 64):
    _c(f"f2.N{_n}", "tn", 33, _n, 70, at=("N > 64",) if _n == 64 else ())
_c("f2.dv", "tn", _T, _HD, _T, TH[::2], geo="dv")
_c("f2.dk", "tn", _T, _HD, _T, TH[::2], geo="dk", alpha=TH_ALPHA)
# --- parts: workgroups per problem, forced (14 row tiles: a wave of the three-way split, 12 tiles a round, still walks two)
# and the heuristic's own on both sides of tiles_m >= 8
PARTS_SHAPES = {0: ("nt", 210, 40, 48), 1: ("nn", 210, 48, 70), 2: ("tn", 210, 48, 70)}
for _f, (_l, _m, _n, _k) in PARTS_SHAPES.items():
    for _p in (1, 2, 3):
        _c(f"parts.f{_f}.hook{_p}", _l, _m, _n, _k, parts=_p, parts_hook=_p)
    _c(f"parts.f{_f}.tiles7", _l, 112, _n, _k, parts=1)
    _c(f"parts.f{_f}.tiles8", _l, 113, _n, _k, parts=1 if _f == 2 else 2)
# (batch >= 4 x the CU count: one workgroup per problem even with eight row tiles; the outer count is the device's CUs)
_c("parts.many_short", "nt", 17, 16, 8, (DEVICE_CUS, 4), parts=1, exact_only=True)
_c("parts.many_tall", "nt", 113, 8, 8, (DEVICE_CUS, 4), parts=1, exact_only=True)
# --- the largest batch build_args admits, on grid.x of the small kernel and on grid.z of the generic one
_c("max_batch.small", "nt", 16, 8, 8, (257, 255), exact_only=True)
_c("max_batch.generic", "nt", 16, 8, 8, (257, 255), path="generic", why="hook", small_hook=0, exact_only=True)
# --- fallback to the generic kernel: one step past each limit
_c("fb.f0.K44", "nt", 33, 40, 44, B35, path="generic", why="form0 K % 8")
_c("fb.f0.K72", "nt", 33, 40, 72, path="generic", why="form0 K > 64")
_c("fb.f0.N688", "nt", 33, 688, 48, path="generic", why="LDS cap")
for _l in ("nn", "tn"):
    _f = {"nn": 1, "tn": 2}[_l]
    _c(f"fb.f{_f}.K257", _l, 33, 48, 257, path="generic", why="K > 256")
    _c(f"fb.f{_f}.N72", _l, 33, 72, 70, path="generic", why="N > 64")
    _c(f"fb.f{_f}.N12", _l, 33, 12, 70, B35, path="generic", why="N % 8")
_c("fb.f2.M257", "tn", 257, 48, 70, path="generic", why="form2 M > 256")
_c("fb.f1.lda197", "nn", 33, 48, 197, path="generic", why="ld % 8", lda=197)
_c("fb.f0.misaligned", "nt", 33, 40, 48, path="generic", why="alignment", a_shift=1)
_c("fb.f0.stride12", "nt", 33, 40, 8, path="generic", why="batch stride", lda=48, a_bs1=12)      # heads of 12 in a row of 36
_c("fb.fp32_in", "nt", 33, 40, 48, path="generic", why="fp32 input", in_bf16=False, c_bf16=False)
_c("fb.fp32_c", "nt", 33, 40, 48, path="generic", why="fp32 C", c_bf16=False)
_c("fb.impl_generic", "nt", 33, 40, 48, path="generic", why="impl", impl=GEMM_GENERIC)
# --- the generic kernel with blockIdx.z > 0
for _l in U.LAYOUTS:
    for _ib in (True, False):
        for _cb in (True, False):
            for _shape in ((130, 75, 40), (333, 129, 65)):
                _c(f"generic.{_l}.{'bf16' if _ib else 'fp32'}.c{'bf16' if _cb else 'fp32'}.{_shape[0]}", _l, *_shape,
                   path="generic", why="impl", impl=GEMM_GENERIC, in_bf16=_ib, c_bf16=_cb)
# (the long op's shapes, reduced: 576 / 784 tokens' P'v and dS k have K > 256, their scores N > 672)
_c("generic.long.nn", "nn", 300, 48, 300, path="generic", why="K > 256")
_c("generic.long.tn", "tn", 300, 48, 300, path="generic", why="K > 256")
_c("generic.long.nt", "nt", 300, 300, 48, path="generic", why="impl", impl=GEMM_GENERIC)

SIX_PRODUCTS = ("f0.scores", "f1.pv", "f0.dpm", "f1.dq", "f2.dv", "f2.dk")     # th_three_call_fwd + _bwd, in call order
# every condition of the dispatch a fallback case must fail.  (gemm_small_form also asks lda >= ru8(K) of form 1 and
# lda >= ru8(M) of form 2; with lda % 8 == 0 asked before and lda >= K / M by build_args these cannot fail.)
CONDITIONS = ("fp32 input", "fp32 C", "ld % 8", "alignment", "batch stride", "form0 K % 8", "form0 K > 64", "N % 8",
              "N > 64", "K > 256", "form2 M > 256", "LDS cap", "impl", "hook")
LIMITS = ("form0 K > 64", "N > 64", "K > 256", "form2 M > 256", "LDS cap")      # ... and those a small case sits on


def exact_cases():
    return list(CASES)


def accuracy_cases():
    return [n for n, c in CASES.items() if not c.exact_only]


def exact_alpha(name):
    """1 or 0.5, in turn down the table."""
    return 0.5 if list(CASES).index(name) % 2 else 1.0


# --------------------------------------------------------------------------------------------- geometry ---
def _op(store, rows, cols, ld, bs, off):
    return SimpleNamespace(store=store, rows=rows, cols=cols, ld=ld, bs=tuple(bs), off=off)


def geometry(case, cus=DEVICE_CUS):
    """Where the operands of `case` lie: .a / .b / .c (store, rows, cols of the STORED matrix, ld, bs, off, in elements)
    and .sizes {store: elements}.  cus: the device's CU count (the outer batch of the parts.many_* cases)."""
    c = case
    akm, bkm = U.LAYOUTS[c.layout]
    outer = cus if c.name.startswith("parts.many") else c.outer
    g = SimpleNamespace(M=c.M, N=c.N, K=c.K, akm=akm, bkm=bkm, outer=outer, inner=c.inner, batch=outer * c.inner)
    ra, ca = (c.M, c.K) if akm else (c.K, c.M)
    rb, cb = (c.N, c.K) if bkm else (c.K, c.N)
    if c.geo == "plain":
        def op(store, rows, cols, ld, gap, shift, bs1=None):
            if bs1 is None:
                bs = (c.inner * (rows * ld + gap) + gap + 8, rows * ld + gap)
            else:                                   # the inner level's problems side by side in one row (heads)
                bs = (rows * ld + gap + 8, bs1)
            return _op(store, rows, cols, ld, bs, FRONT + shift)
        g.a = op("a", ra, ca, c.lda or ru(ca, 8) + 8, 16, c.a_shift, c.a_bs1)
        g.b = op("b", rb, cb, ru(cb, 8) + 24, 16, 0)
        g.c = op("c", c.M, c.N, c.ldc or ru(c.N, 8) + 8, 8, c.c_shift)
    else:
        T, H, hd = c.M, c.inner, (c.K if c.geo in ("scores", "dpm") else c.N)
        D, D3, NS = H * hd, 3 * H * hd, ru(T, 8)
        qkv = lambda third: _op("qkv", T, hd, D3, (T * D3, hd), FRONT + third * D)
        do = lambda store: _op(store, T, hd, D, (T * D, hd), FRONT)
        s = lambda: _op("s", T, T, NS, (H * T * NS, T * NS), FRONT)
        g.a, g.b, g.c = {"scores": (qkv(0), qkv(1), s()), "dpm": (do("do"), qkv(2), s()), "pv": (s(), qkv(2), do("o")),
                         "dq": (s(), qkv(1), qkv(0)), "dv": (s(), do("do"), qkv(2)), "dk": (s(), qkv(0), qkv(1))}[c.geo]
        if g.c.store == "qkv":
            g.c.store = "dqkv"
    g.sizes = {}
    for o in (g.a, g.b, g.c):
        end = o.off + (outer - 1) * o.bs[0] + (c.inner - 1) * o.bs[1] + (o.rows - 1) * o.ld + o.cols + TAIL
        g.sizes[o.store] = max(g.sizes.get(o.store, 0), end)
    return g


def window_index(o, outer, inner):
    """Element index of (problem, row, col) of operand `o` in its storage: int64 [outer * inner, rows, cols]."""
    ar = lambda n: torch.arange(n, dtype=torch.int64)
    z = (ar(outer)[:, None] * o.bs[0] + ar(inner)[None, :] * o.bs[1]).reshape(-1)
    return o.off + z[:, None, None] + ar(o.rows)[None, :, None] * o.ld + ar(o.cols)[None, None, :]


def build_storages(g, a_stored, b_stored, in_dtype, c_dtype, device="cpu"):
    """{store: flat NaN-filled tensor} with the batch's operands written into their windows (the output's storage is all
    NaN), and the output's window index."""
    st = {}
    for o, mats, dt in ((g.a, a_stored, in_dtype), (g.b, b_stored, in_dtype), (g.c, None, c_dtype)):
        if o.store not in st:
            st[o.store] = torch.full((g.sizes[o.store],), float("nan"), dtype=dt)
        if mats is not None:
            st[o.store][window_index(o, g.outer, g.inner).reshape(-1)] = mats.reshape(-1).to(dt)
    return {k: v.to(device) for k, v in st.items()}, window_index(g.c, g.outer, g.inner)


def read_windows(cbuf, idx):
    """(the batch's outputs [batch, M, N], is everything outside the windows still NaN?) of the output storage on the CPU."""
    outside = torch.ones(cbuf.numel(), dtype=torch.bool)
    outside[idx.reshape(-1)] = False
    return cbuf[idx.reshape(-1)].view(idx.shape), bool(torch.isnan(cbuf[outside].float()).all())


def descriptor(case, g, base, alpha):
    """The vitmi_gemm_desc of the call; base: {store: address of the storage's first element}."""
    from vit_torch_amd._lib import GemmDesc
    es = 2 if case.in_bf16 else 4
    d = GemmDesc()
    d.M, d.N, d.K = g.M, g.N, g.K
    d.A, d.lda, d.a_kmajor = base[g.a.store] + g.a.off * es, g.a.ld, int(g.akm)
    d.B, d.ldb, d.b_kmajor = base[g.b.store] + g.b.off * es, g.b.ld, int(g.bkm)
    d.C, d.ldc = base[g.c.store] + g.c.off * (2 if case.c_bf16 else 4), g.c.ld
    d.in_dtype, d.c_dtype = (BF16_CODE if case.in_bf16 else F32_CODE), (BF16_CODE if case.c_bf16 else F32_CODE)
    d.epilogue, d.alpha, d.impl = U.EPI_STORE, float(alpha), case.impl
    d.batch, d.batch_inner = g.batch, g.inner
    for f, o in (("a_bs", g.a), ("b_bs", g.b), ("c_bs", g.c)):
        getattr(d, f)[0], getattr(d, f)[1] = o.bs
    return d


# ----------------------------------------------------------------------------- the dispatch, mirrored ---
def small_form(case, g):
    """(form, None) if the call takes gemm_small.hip, else (-1, the first condition it fails): choose_path's batched
    branch, gemm_small_form and small_lds_ok line by line.  Storages start 16-byte aligned."""
    es = 2 if case.in_bf16 else 4
    if case.small_hook == 0:
        return -1, "hook"
    if case.impl == GEMM_GENERIC and case.small_hook != 1:
        return -1, "impl"
    if not case.in_bf16:
        return -1, "fp32 input"
    if g.batch <= 1:
        return -1, "batch"
    if not case.c_bf16:
        return -1, "fp32 C"
    if g.a.ld % 8 or g.b.ld % 8:
        return -1, "ld % 8"
    if (g.a.off * es) % 16 or (g.b.off * es) % 16:
        return -1, "alignment"
    if any(s % 8 for s in g.a.bs + g.b.bs):
        return -1, "batch stride"
    if g.akm and g.bkm:
        if g.K % 8:
            return -1, "form0 K % 8"
        if g.K > 64:
            return -1, "form0 K > 64"
        form = 0
    else:
        if g.N % 8:
            return -1, "N % 8"
        if g.N > SB_MAXN:
            return -1, "N > 64"
        if g.K > SB_MAXK:
            return -1, "K > 256"
        if g.akm and not g.bkm:
            if g.a.ld < ru(g.K, 8):
                return -1, "lda < ru8(K)"
            form = 1
        elif not g.akm and not g.bkm:
            if g.a.ld < ru(g.M, 8):
                return -1, "lda < ru8(M)"
            if g.M > 256:
                return -1, "form2 M > 256"
            form = 2
        else:
            return -1, "layout tt"
    if small_lds(form, g.M, g.N, g.K) > LDS_CAP:
        return -1, "LDS cap"
    return form, None


def small_lds(form, M, N, K):
    """Dynamic LDS of gemm_small_kernel<form> in bytes."""
    if form == 0:
        return ru(N, 16) * (64 * 2 + 16)
    pitch = lambda cols: cols * 2 + (32 if (cols * 2) % 128 == 0 else 0)
    return ru(K, 32) * pitch(ru(N, 16)) + (SB_CHUNK * pitch(ru(M, 16)) if form == 2 else 0)


def small_parts(case, g, form, cus=DEVICE_CUS):
    """gemm_small_parts: the workgroups that share one problem."""
    if case.parts_hook > 0:
        return case.parts_hook
    return 2 if form != 2 and g.batch < 4 * cus and ru(g.M, 16) // 16 >= 8 else 1


def expected_plan(case, g, cus=DEVICE_CUS):
    """(path, form, parts) as vitmi_debug_gemm_path reports them."""
    form, _ = small_form(case, g)
    if form < 0:
        return PATH_GENERIC, -1, 0
    return PATH_SMALL, form, small_parts(case, g, form, cus)


# ------------------------------------------------------------------------------- inputs and reference ---
@functools.lru_cache(maxsize=8)
def problem(name, family, cus=DEVICE_CUS):
    """The batch's inputs and float64 products, computed once per (case, family): .a [batch, M, K], .b [batch, N, K]
    (logical, k-major, float64 values exact in the input dtype), .prod [batch, M, N] = a b^T per problem in float64
    (gemm_util.product), .norm [M, N].  One seeded stream feeds the whole batch, so every problem has operands of its own:
    a problem computed from another one's is off by integers in the `integer` family.  `scaled`: gemm_util's row scales
    2^((m mod 7) - 3) on a and 2^((n mod 5) - 2) on b within every problem."""
    c = CASES[name]
    g = geometry(c, cus)
    seed = zlib.crc32(name.encode()) % 100003 + (7 if family == "scaled" else 0)
    fam = "normal" if family == "scaled" else family
    a = U.make_inputs(fam, g.batch * c.M, 1, c.K, None, seed, in_bf16=c.in_bf16)["a"].view(g.batch, c.M, c.K)
    b = U.make_inputs(fam, 1, g.batch * c.N, c.K, None, seed + 1, in_bf16=c.in_bf16)["b"].view(g.batch, c.N, c.K)
    norm = torch.ones((c.M, c.N), dtype=F64)
    if family == "scaled":
        sa, sb = U.row_scales(c.M, 7, 3), U.row_scales(c.N, 5, 2)
        a, b, norm = a * sa[None, :, None], b * sb[None, :, None], sa[:, None] * sb[None, :]
    if g.batch <= 64:
        prod = torch.stack([U.product(a[z], b[z]) for z in range(g.batch)])
    else:
        prod = torch.bmm(a, b.transpose(1, 2))
    return SimpleNamespace(a=a, b=b, prod=prod, norm=norm)


def stored(p, g):
    """The operands as the layout stores them: A [batch, M, K] or [batch, K, M], B [batch, N, K] or [batch, K, N]."""
    return (p.a if g.akm else p.a.transpose(1, 2)), (p.b if g.bkm else p.b.transpose(1, 2))


def want(p, alpha):
    """The float64 reference: alpha (the float32 value the descriptor carries) times the product, in float64."""
    return p.prod * float(torch.tensor(alpha, dtype=torch.float32))
