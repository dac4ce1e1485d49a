"""Tensor-level wrappers over the C ABI (include/vitmi.h).

PyTorch is used here only for device memory and the current HIP stream; every
function enqueues hand-written HIP kernels from libvitmi.so and nothing else.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import (BF16, EPI_BIAS_GELU, EPI_DGELU, EPI_PATCH_POS, EPI_RESIDUAL, EPI_STORE, F32,
                   GEMM_AUTO, GEMM_FAST, GEMM_GENERIC, FoldDesc, GemmDesc, check, load)

_WS: dict = {}


def dtype_code_or_neg(t) -> int:
    """The ABI's dtype code (BF16 / F32) of a tensor or a torch.dtype, -1 for a dtype the library does not take: what the
    host-only `*_supported` queries pass on."""
    dt = t if isinstance(t, torch.dtype) else t.dtype
    return BF16 if dt == torch.bfloat16 else F32 if dt == torch.float32 else -1


def dtype_code(t: torch.Tensor) -> int:
    code = dtype_code_or_neg(t)
    if code < 0:
        raise TypeError(f"vitmi: unsupported dtype {t.dtype}")
    return code


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.VitmiError("vitmi ops run on the GPU only (tensor is on %s); there is no CPU fallback" % t.device)


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer per (device, stream)."""
    key = (str(device), _stream())
    w = _WS.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = w
    return w


def _aligned_ws(need: int, device, none_if_unneeded=False):
    """`need` bytes of the workspace behind a 256-byte-aligned address: (pointer, bytes from there on); (None, 0) for
    need == 0 where the kernel family takes "no workspace" that way."""
    if none_if_unneeded and not need:
        return None, 0
    w = workspace(need + 256, device)
    off = (-w.data_ptr()) % 256
    return w.data_ptr() + off, w.numel() - off


def _contract(who, name, t, dtype, numel, shape):
    """A tensor argument's contract: contiguous, `dtype`, `numel` elements (`shape`: the expected shape, as text)."""
    if t.dtype != dtype or not t.is_contiguous() or t.numel() != numel:
        raise _lib.VitmiError(f"{who}: {name} must be a contiguous {dtype} {shape} tensor (got {t.dtype}, {tuple(t.shape)})")


def gemm(A, B, C_out, **k):
    """C = epilogue(op(A) @ op(B)^T); see vitmi_gemm in include/vitmi.h.  The keywords are _gemm_desc's."""
    d = _gemm_desc(A, B, C_out, **k)
    lib = load()
    need = lib.vitmi_gemm_workspace(C.byref(d))
    if need:
        ws = workspace(need, A.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    check(lib.vitmi_gemm(C.byref(d), _stream()), "vitmi_gemm")
    return C_out


def split3(x, *, b_pattern: bool, stacked: bool):
    """The bf16 image of an fp32 matrix for the "bf16x3" mode (vitmi_split3): [rows, 3 cols] (k-major operand) or
    [3 rows, cols] (k-minor operand), A pattern hi|lo|hi or B pattern hi|hi|lo."""
    _need_cuda(x)
    assert x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1
    R, Cn = x.shape
    out = torch.empty((3 * R, Cn) if stacked else (R, 3 * Cn), dtype=torch.bfloat16, device=x.device)
    check(load().vitmi_split3(x.data_ptr(), x.stride(0), R, Cn, out.data_ptr(), out.stride(0), int(b_pattern), int(stacked),
                              _stream()), "vitmi_split3")
    return out


def gelu_fwd(pre, out):
    _need_cuda(pre, out)
    M, N = pre.shape
    check(load().vitmi_gelu_fwd(pre.data_ptr(), pre.stride(0), out.data_ptr(), out.stride(0), M, N, _stream()), "vitmi_gelu_fwd")
    return out


def gelu_bwd(dh, pre, out):
    _need_cuda(dh, pre, out)
    M, N = pre.shape
    check(load().vitmi_gelu_bwd(dh.data_ptr(), dh.stride(0), pre.data_ptr(), pre.stride(0), out.data_ptr(), out.stride(0),
                                M, N, _stream()), "vitmi_gelu_bwd")
    return out


def gemm_split3(A, B, C_out, *, a_kmajor=True, b_kmajor=True, epilogue=EPI_STORE, bias=None, aux=None, C2=None,
                aux_deriv=False, colsum_part=None, **k):
    """`gemm` for fp32 operands in the "bf16x3" mode: both operands are written as their three-part bf16 images
    (`split3`) and ONE bf16 product over K' = 3K runs on the tile kernels with the fp32 epilogue asked for.  The two GELU
    epilogues (bf16-only on the tile kernel) become a plain fp32 product + the element-wise fp32 kernel."""
    assert A.dtype == torch.float32 and B.dtype == torch.float32 and C_out.dtype == torch.float32
    assert colsum_part is None and not aux_deriv
    A3 = split3(A, b_pattern=False, stacked=not a_kmajor)
    B3 = split3(B, b_pattern=True, stacked=not b_kmajor)
    if epilogue == EPI_BIAS_GELU:
        pre = C2 if C2 is not None else torch.empty_like(C_out)
        gemm(A3, B3, pre, a_kmajor=a_kmajor, b_kmajor=b_kmajor, bias=bias, **k)
        return gelu_fwd(pre, C_out)
    if epilogue == EPI_DGELU:
        gemm(A3, B3, C_out, a_kmajor=a_kmajor, b_kmajor=b_kmajor, **k)
        return gelu_bwd(C_out, aux, C_out)
    return gemm(A3, B3, C_out, a_kmajor=a_kmajor, b_kmajor=b_kmajor, epilogue=epilogue, bias=bias, C2=C2, **k)


def gemm_pair(A0, B0, C0, A1, B1, C1, launch_flags=0):
    """Two weight-gradient products C_i = A_i^T @ B_i (k-minor operands [tokens, features], fp32 C) in one launch where
    the library can pair them (vitmi_gemm_pair), else one after the other; same results."""
    d0 = _gemm_desc(A0, B0, C0, a_kmajor=False, b_kmajor=False, launch_flags=launch_flags)
    d1 = _gemm_desc(A1, B1, C1, a_kmajor=False, b_kmajor=False, launch_flags=launch_flags)
    lib = load()
    need = max(lib.vitmi_gemm_pair_workspace(C.byref(d0), C.byref(d1)), lib.vitmi_gemm_workspace(C.byref(d0)),
               lib.vitmi_gemm_workspace(C.byref(d1)))
    ws = workspace(need, A0.device)
    for d in (d0, d1):                       # the fallback (two vitmi_gemm calls) splits K through the descriptors' own fields
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    check(lib.vitmi_gemm_pair(C.byref(d0), C.byref(d1), ws.data_ptr(), ws.numel(), _stream()), "vitmi_gemm_pair")


def gemm_pair_shares_a_launch(M0, N0, M1, N1, K) -> bool:
    """Host-only query: would the two k-minor bf16 products [M0,N0] and [M1,N1] over K rows share one launch?"""
    ds = []
    for M, N in ((M0, N0), (M1, N1)):
        d = GemmDesc()
        d.M, d.N, d.K = M, N, K
        d.A = d.B = d.C = 256
        d.lda, d.ldb, d.ldc = M, N, N
        d.a_kmajor = d.b_kmajor = 0
        d.in_dtype, d.c_dtype, d.epilogue = BF16, F32, EPI_STORE
        ds.append(d)
    return load().vitmi_gemm_pair_workspace(C.byref(ds[0]), C.byref(ds[1])) > 0


def _gemm_desc(A, B, C_out, *, a_kmajor=True, b_kmajor=True, epilogue=EPI_STORE, bias=None, R=None,
               gamma=None, aux=None, C2=None, pos=None, n_tok=0, cls=None, alpha=1.0, accumulate=False,
               impl=GEMM_AUTO, rowscale=None, rows_per_group=0, colsum_part=None, aux_deriv=False,
               launch_flags=0):
    """The vitmi_gemm_desc of one product (include/vitmi.h describes each field).  a_kmajor / b_kmajor: the operand is
    [rows, K] (else [K, rows]); epilogue: EPI_*; bias [N], gamma [N] (LayerScale), cls [N], pos [n_tok * N]: fp32 vectors of
    the epilogues; R: the residual [M, N]; aux: the saved pre-activation (or, with aux_deriv, its gelu') of EPI_DGELU;
    C2: a second [M, N] output (the pre-activation / gelu' of EPI_BIAS_GELU, the branch output of EPI_RESIDUAL);
    alpha: scale of the product; accumulate: C += ; impl: GEMM_AUTO / _FAST / _GENERIC; rowscale [>= M / rows_per_group]:
    DropPath's per-sample scale; colsum_part [ceil(M / 128), N]: per-128-row column sums of C; launch_flags: VITMI_LAUNCH_*."""
    _need_cuda(A, B, C_out)
    assert A.dim() == 2 and B.dim() == 2 and C_out.dim() == 2
    assert A.stride(1) == 1 and B.stride(1) == 1 and C_out.stride(1) == 1
    M, K = (A.shape if a_kmajor else (A.shape[1], A.shape[0]))
    N, Kb = (B.shape if b_kmajor else (B.shape[1], B.shape[0]))
    assert K == Kb, f"gemm: K mismatch {K} vs {Kb}"
    assert tuple(C_out.shape) == (M, N), f"gemm: C shape {tuple(C_out.shape)} != {(M, N)}"
    assert A.dtype == B.dtype
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.A, d.lda, d.a_kmajor = A.data_ptr(), A.stride(0), int(a_kmajor)
    d.B, d.ldb, d.b_kmajor = B.data_ptr(), B.stride(0), int(b_kmajor)
    d.in_dtype = dtype_code(A)
    d.epilogue = epilogue
    d.C, d.ldc, d.c_dtype = C_out.data_ptr(), C_out.stride(0), dtype_code(C_out)
    if C2 is not None:
        want = A.dtype if epilogue == EPI_RESIDUAL else C_out.dtype
        assert C2.dtype == want and tuple(C2.shape) == (M, N) and C2.stride(1) == 1
        d.C2, d.ldc2 = C2.data_ptr(), C2.stride(0)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous()
        d.bias = bias.data_ptr()
    if R is not None:
        assert tuple(R.shape) == (M, N) and R.stride(1) == 1
        d.R, d.ldr, d.r_dtype = R.data_ptr(), R.stride(0), dtype_code(R)
    if gamma is not None:
        assert gamma.dtype == torch.float32 and gamma.numel() == N and gamma.is_contiguous()
        d.gamma = gamma.data_ptr()
    if aux is not None:
        assert aux.dtype == A.dtype and tuple(aux.shape) == (M, N) and aux.stride(1) == 1
        d.AUX, d.ldaux = aux.data_ptr(), aux.stride(0)
    if pos is not None:
        assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.numel() == n_tok * N
        d.pos, d.n_tok = pos.data_ptr(), n_tok
    if cls is not None:
        assert cls.dtype == torch.float32 and cls.numel() == N and cls.is_contiguous()
        d.cls = cls.data_ptr()
    d.alpha = float(alpha)
    d.accumulate = int(accumulate)
    d.impl = impl
    if rowscale is not None:
        assert rowscale.dtype == torch.float32 and rows_per_group > 0 and rowscale.numel() * rows_per_group >= M
        d.rowscale, d.rows_per_group = rowscale.data_ptr(), rows_per_group
    if colsum_part is not None:
        assert colsum_part.dtype == torch.float32 and colsum_part.is_contiguous()
        assert tuple(colsum_part.shape) == ((M + 127) // 128, N)
        d.colsum_part = colsum_part.data_ptr()
    d.aux_is_derivative = int(bool(aux_deriv))
    d.launch_flags = int(launch_flags)
    return d


def gemm_batched(A, B, C_out, *, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, batch, batch_inner,
                 a_bs, b_bs, c_bs, a_off=0, b_off=0, c_off=0, alpha=1.0, impl=GEMM_AUTO):
    """batch independent products on strided views of A/B/C storage (element offsets/strides):
    C_z = alpha * op(A_z) op(B_z)^T, z = zo*batch_inner + zi.  One workgroup per problem for
    small bf16 problems (gemm_small.hip), else the generic MFMA kernel (impl=GEMM_GENERIC forces it)."""
    _need_cuda(A, B, C_out)
    assert A.dtype == B.dtype
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.A, d.lda, d.a_kmajor = A.data_ptr() + a_off * A.element_size(), lda, int(a_kmajor)
    d.B, d.ldb, d.b_kmajor = B.data_ptr() + b_off * B.element_size(), ldb, int(b_kmajor)
    d.in_dtype = dtype_code(A)
    d.epilogue = EPI_STORE
    d.C, d.ldc, d.c_dtype = C_out.data_ptr() + c_off * C_out.element_size(), ldc, dtype_code(C_out)
    d.alpha = float(alpha)
    d.impl = impl
    d.batch, d.batch_inner = batch, batch_inner
    d.a_bs[0], d.a_bs[1] = a_bs
    d.b_bs[0], d.b_bs[1] = b_bs
    d.c_bs[0], d.c_bs[1] = c_bs
    check(load().vitmi_gemm(C.byref(d), _stream()), "vitmi_gemm(batched)")
    return C_out


def gemm_uses_fast(M, N, K, *, a_kmajor=True, b_kmajor=True, in_dtype=BF16, c_dtype=BF16,
                   epilogue=EPI_STORE, lda=None, ldb=None, ldc=None, colsum_part=False, launch_flags=0) -> bool:
    """Host-only query (no GPU needed): would this problem take the fast kernel?  launch_flags: VITMI_LAUNCH_*, as the
    call itself would pass them."""
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.A = d.B = d.C = 256  # any non-null, 256-B aligned address
    d.R = d.AUX = d.pos = 256
    d.lda = lda or (K if a_kmajor else M)
    d.ldb = ldb or (K if b_kmajor else N)
    d.ldc = ldc or N
    d.ldr = d.ldaux = N
    d.n_tok = 1
    d.a_kmajor, d.b_kmajor = int(a_kmajor), int(b_kmajor)
    d.in_dtype, d.c_dtype, d.r_dtype, d.epilogue = in_dtype, c_dtype, c_dtype, epilogue
    if colsum_part:
        d.colsum_part = 256
    d.launch_flags = int(launch_flags)
    return bool(load().vitmi_gemm_uses_fast(C.byref(d)))


def layernorm_fwd(x, gamma, beta, y, mean, rstd, eps, *, M=None, D=None, x_stride=None, y_stride=None):
    """Rows of x (stride x_stride elements) -> y; mean/rstd fp32 [M] (may be None)."""
    _need_cuda(x, y)
    D = D or x.shape[-1]
    M = M or x.numel() // D
    xs = x_stride if x_stride is not None else D
    ys = y_stride if y_stride is not None else D
    check(load().vitmi_layernorm_fwd(x.data_ptr(), dtype_code(x), xs, gamma.data_ptr(), beta.data_ptr(),
                                     y.data_ptr(), dtype_code(y), ys, _ptr(mean), _ptr(rstd),
                                     M, D, float(eps), _stream()), "vitmi_layernorm_fwd")
    return y


class FoldQueue:
    """Deferred folds of fp32 partial column sums (vitmi_fold_many): the engines queue the ~50 small folds of a backward
    pass (LayerNorm dgamma | dbeta | bias sums, the bias partials of the GEMM / attention epilogues) and run them in one
    launch per flush — at the end of backward, or before a gradient-bucket section is handed to the reducer.  The queue
    keeps the partial buffers alive until then.  Results are bit-identical to the single folds."""

    def __init__(self):
        self._descs, self._keep = [], []

    def add(self, part, S, N, ld, outs, keep=()):
        d = FoldDesc()
        d.part, d.S, d.nseg, d.N, d.ld = part.data_ptr(), int(S), len(outs), int(N), int(ld)
        for k, o in enumerate(outs):
            assert o.dtype == torch.float32 and o.numel() >= N
            d.out[k] = o.data_ptr()
        self._descs.append(d)
        self._keep.append((part, outs, keep))

    def add_desc(self, d, keep):
        self._descs.append(d)
        self._keep.append(keep)

    def __len__(self):
        return len(self._descs)

    def flush(self):
        if not self._descs:
            return
        arr = (FoldDesc * len(self._descs))(*self._descs)
        try:
            check(load().vitmi_fold_many(arr, len(self._descs), _stream()), "vitmi_fold_many")
        finally:
            self._descs, self._keep = [], []

    def clear(self):
        self._descs, self._keep = [], []


def layernorm_bwd(dy, x, mean, rstd, gamma, g_in, g_out, gb_out, dgamma, dbeta, *, gsum=None,
                  gb_scale=None, gb_rowscale=None, rows_per_group=0, M=None, D=None, dy_stride=None,
                  x_stride=None, g_stride=None, gb_stride=None, fold=None):
    """fold (a FoldQueue): leave the fold of the dgamma | dbeta | gsum partials to the queue's next flush; the partial
    rows then live in a buffer of their own (kept by the queue) instead of the shared workspace."""
    _need_cuda(dy, x, g_out)
    D = D or x.shape[-1]
    M = M or dy.numel() // D
    lib = load()
    nbytes = lib.vitmi_layernorm_bwd_workspace(M, D)
    args = (
        dy.data_ptr(), dtype_code(dy), dy_stride if dy_stride is not None else D,
        x.data_ptr(), dtype_code(x), x_stride if x_stride is not None else D,
        mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
        _ptr(g_in), g_out.data_ptr(), dtype_code(g_out), g_stride if g_stride is not None else D,
        _ptr(gb_out), dtype_code(gb_out) if gb_out is not None else dtype_code(dy),
        gb_stride if gb_stride is not None else D,
        dgamma.data_ptr(), dbeta.data_ptr(), _ptr(gsum), _ptr(gb_scale), _ptr(gb_rowscale), rows_per_group,
        M, D)
    if fold is None:
        ws = workspace(nbytes, dy.device)
        check(lib.vitmi_layernorm_bwd(*args, ws.data_ptr(), ws.numel(), _stream()), "vitmi_layernorm_bwd")
        return
    part = torch.empty(int(nbytes), dtype=torch.uint8, device=dy.device)
    d = FoldDesc()
    check(lib.vitmi_layernorm_bwd_deferred(*args, part.data_ptr(), part.numel(), C.byref(d), _stream()),
          "vitmi_layernorm_bwd_deferred")
    fold.add_desc(d, (part, dgamma, dbeta, gsum))


def attn_fwd(qkv, out, lse, B, N, H, hd, scale):
    _need_cuda(qkv, out, lse)
    assert qkv.is_contiguous() and out.is_contiguous() and lse.dtype == torch.float32
    check(load().vitmi_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), dtype_code(qkv),
                                B, N, H, hd, float(scale), _stream()), "vitmi_attn_fwd")
    return out


def attn_probs(qkv, P, B, N, H, hd, scale):
    """P [B, H, N, N] fp32 = softmax((q k^T) * scale) of qkv [B*N, 3*H*hd] (bf16 or fp32, as attn_fwd reads it):
    the attention probabilities materialised (vitmi_attn_probs; DINO's get_last_selfattention).  Forward only."""
    _need_cuda(qkv, P)
    if qkv.dtype not in (torch.bfloat16, torch.float32):
        raise _lib.VitmiError(f"attn_probs: qkv must be bf16 or fp32, got {qkv.dtype}")
    if P.dtype != torch.float32 or not P.is_contiguous() or P.numel() != B * H * N * N:
        raise _lib.VitmiError(f"attn_probs: P must be a contiguous fp32 [B, H, N, N] = [{B}, {H}, {N}, {N}] tensor "
                              f"(got {P.dtype}, {tuple(P.shape)})")
    if not qkv.is_contiguous() or qkv.numel() != B * N * 3 * H * hd:
        raise _lib.VitmiError(f"attn_probs: qkv must be a contiguous [B*N, 3*H*hd] = [{B * N}, {3 * H * hd}] tensor "
                              f"(got {tuple(qkv.shape)})")
    check(load().vitmi_attn_probs(qkv.data_ptr(), P.data_ptr(), dtype_code(qkv), B, N, H, hd, float(scale), _stream()),
          "vitmi_attn_probs")
    return P


def xca_supported(t, H, N, hd) -> bool:
    """Host-only query: do the cross-covariance attention kernels (xca_fwd / xca_bwd) take this dtype and shape?"""
    return bool(load().vitmi_xca_supported(dtype_code_or_neg(t), H, N, hd))


def _xca_check(who, qkv, temperature, B, N, H, hd):
    if qkv.dtype not in (torch.bfloat16, torch.float32):
        raise _lib.VitmiError(f"{who}: qkv must be bf16 or fp32, got {qkv.dtype}")
    _contract(who, "qkv", qkv, qkv.dtype, B * N * 3 * H * hd, f"[B*N, 3*H*hd] = [{B * N}, {3 * H * hd}]")
    _contract(who, "temperature", temperature, torch.float32, H, f"[H] = [{H}]")


def xca_fwd(qkv, temperature, out, stat, B, N, H, hd):
    """out [B, N, H*hd] = XCiT's cross-covariance attention of qkv [B*N, 3*H*hd] (bf16 or fp32, as attn_fwd reads it) with
    the per-head fp32 temperature [H]; stat fp32 [B, H, hd+2, hd] (normalised covariance and both norm rows) is what
    xca_bwd needs besides qkv (vitmi_xca_fwd).  hd in {32, 48, 64}."""
    _need_cuda(qkv, temperature, out, stat)
    _xca_check("xca_fwd", qkv, temperature, B, N, H, hd)
    _contract("xca_fwd", "out", out, qkv.dtype, B * N * H * hd, f"[B, N, H*hd] = [{B}, {N}, {H * hd}]")
    _contract("xca_fwd", "stat", stat, torch.float32, B * H * (hd + 2) * hd, f"[B, H, hd+2, hd] = [{B}, {H}, {hd + 2}, {hd}]")
    ptr, nb = _aligned_ws(load().vitmi_xca_workspace(B, H, N, hd), qkv.device, none_if_unneeded=True)
    check(load().vitmi_xca_fwd(qkv.data_ptr(), temperature.data_ptr(), out.data_ptr(), stat.data_ptr(), dtype_code(qkv),
                               B, N, H, hd, ptr, nb, _stream()), "vitmi_xca_fwd")
    return out


def xca_bwd(qkv, dout, temperature, stat, dqkv, dtemp, B, N, H, hd):
    """Backward of xca_fwd: dqkv [B*N, 3*H*hd] and dtemp fp32 [H] from dout [B, N, H*hd] (vitmi_xca_bwd writes one
    temperature partial per (image, head); their batch sum is a colsum)."""
    _need_cuda(qkv, dout, temperature, stat, dqkv, dtemp)
    _xca_check("xca_bwd", qkv, temperature, B, N, H, hd)
    _contract("xca_bwd", "dout", dout, qkv.dtype, B * N * H * hd, f"[B, N, H*hd] = [{B}, {N}, {H * hd}]")
    _contract("xca_bwd", "dqkv", dqkv, qkv.dtype, B * N * 3 * H * hd, f"[B*N, 3*H*hd] = [{B * N}, {3 * H * hd}]")
    _contract("xca_bwd", "stat", stat, torch.float32, B * H * (hd + 2) * hd, f"[B, H, hd+2, hd] = [{B}, {H}, {hd + 2}, {hd}]")
    _contract("xca_bwd", "dtemp", dtemp, torch.float32, H, f"[H] = [{H}]")
    part = torch.empty((B, H), dtype=torch.float32, device=qkv.device)
    ptr, nb = _aligned_ws(load().vitmi_xca_workspace(B, H, N, hd), qkv.device, none_if_unneeded=True)
    check(load().vitmi_xca_bwd(qkv.data_ptr(), dout.data_ptr(), temperature.data_ptr(), stat.data_ptr(), dqkv.data_ptr(),
                               part.data_ptr(), dtype_code(qkv), B, N, H, hd, ptr, nb, _stream()), "vitmi_xca_bwd")
    colsum(part, dtemp, M=B, N=H)
    return dqkv


def lpi_supported(t, B, H, W, C) -> bool:
    """Host-only query: do the local patch interaction kernels (lpi_fwd / lpi_bwd) take this dtype and shape?"""
    return bool(load().vitmi_lpi_supported(dtype_code_or_neg(t), B, H, W, C))


def _lpi_contract(who, x, acts, f32s, B, H, W, C):
    """lpi_fwd / lpi_bwd: x is bf16 or fp32; `acts` (name, tensor) are [B, H*W, C] in x's dtype; `f32s` (name, tensor,
    elements) are fp32 (a None tensor is an optional one left out)."""
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise _lib.VitmiError(f"{who}: x must be bf16 or fp32, got {x.dtype}")
    for name, t in acts:
        _contract(who, name, t, x.dtype, B * H * W * C, f"[B, H*W, C] = [{B}, {H * W}, {C}]")
    for name, t, n in f32s:
        if t is not None:
            _contract(who, name, t, torch.float32, n, f"{n}-element")


def lpi_fwd(x, w1, b1, gamma, beta, w2, b2, running_mean, running_var, num_batches_tracked, u, stat, out, B, H, W, C, *,
            training, momentum=0.1, eps=1e-5):
    """out [B, H*W, C] = XCiT's LPI (depthwise 3x3 conv, GELU, BatchNorm2d, depthwise 3x3 conv) of the token-major
    x [B, H*W, C] (bf16 or fp32); fp32 parameters, the conv weights as their own [C,1,3,3] memory.  Writes u (the GELU
    output, compute dtype) and stat fp32 [2, C] (mean, rstd), which lpi_bwd needs.  training: batch statistics, and the
    three running buffers (fp32 [C], fp32 [C], int64 [1]; each may be None) are updated on the device; otherwise the
    running statistics are used and nothing is touched (vitmi_lpi_fwd)."""
    _need_cuda(x, w1, b1, gamma, beta, w2, b2, running_mean, running_var, num_batches_tracked, u, stat, out)
    _lpi_contract("lpi_fwd", x, (("x", x), ("u", u), ("out", out)),
                  (("conv1.weight", w1, 9 * C), ("conv1.bias", b1, C), ("bn.weight", gamma, C), ("bn.bias", beta, C),
                   ("conv2.weight", w2, 9 * C), ("conv2.bias", b2, C), ("stat", stat, 2 * C),
                   ("running_mean", running_mean, C), ("running_var", running_var, C)), B, H, W, C)
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1):
        raise _lib.VitmiError("lpi_fwd: num_batches_tracked must be an int64 tensor of one element")
    if not training and (running_mean is None or running_var is None):
        raise _lib.VitmiError("lpi_fwd: eval mode needs running_mean and running_var")
    code = dtype_code(x)
    ptr, nb = _aligned_ws(load().vitmi_lpi_workspace(code, B, H, W, C), x.device)
    check(load().vitmi_lpi_fwd(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w2.data_ptr(),
                               b2.data_ptr(), _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), u.data_ptr(),
                               stat.data_ptr(), out.data_ptr(), code, int(bool(training)), momentum, eps, B, H, W, C,
                               ptr, nb, _stream()), "vitmi_lpi_fwd")
    return out


def lpi_bwd(x, u, dout, stat, w1, b1, gamma, beta, w2, dx, dw1, db1, dgamma, dbeta, dw2, db2, B, H, W, C, *, training):
    """Backward of lpi_fwd: dx (compute dtype) and the six fp32 parameter gradients, stored, from dout, the saved u and stat
    and x (vitmi_lpi_bwd); training=False is the eval-mode gradient."""
    _need_cuda(x, u, dout, stat, w1, b1, gamma, beta, w2, dx, dw1, db1, dgamma, dbeta, dw2, db2)
    _lpi_contract("lpi_bwd", x, (("x", x), ("u", u), ("dout", dout), ("dx", dx)),
                  (("stat", stat, 2 * C), ("conv1.weight", w1, 9 * C), ("conv1.bias", b1, C), ("bn.weight", gamma, C),
                   ("bn.bias", beta, C), ("conv2.weight", w2, 9 * C), ("dw1", dw1, 9 * C), ("db1", db1, C),
                   ("dgamma", dgamma, C), ("dbeta", dbeta, C), ("dw2", dw2, 9 * C), ("db2", db2, C)), B, H, W, C)
    code = dtype_code(x)
    ptr, nb = _aligned_ws(load().vitmi_lpi_workspace(code, B, H, W, C), x.device)
    check(load().vitmi_lpi_bwd(x.data_ptr(), u.data_ptr(), dout.data_ptr(), stat.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                               gamma.data_ptr(), beta.data_ptr(), w2.data_ptr(), dx.data_ptr(), dw1.data_ptr(), db1.data_ptr(),
                               dgamma.data_ptr(), dbeta.data_ptr(), dw2.data_ptr(), db2.data_ptr(), code, int(bool(training)),
                               B, H, W, C, ptr, nb, _stream()), "vitmi_lpi_bwd")
    return dx


def conv3s2_supported(t, B, H, W, C, ld, *, image=False) -> bool:
    """Host-only query: do conv3s2_im2col (image: its fp32-image form) / conv3s2_col2im take this compute dtype and shape?"""
    return bool(load().vitmi_conv3s2_supported(dtype_code_or_neg(t), int(bool(image)), B, H, W, C, ld))


def _conv3s2_check(who, t, B, H, W, C, ld, image):
    """The supported query before anything else, so that an unsupported dtype or shape raises VitmiError with the library's
    own message, and the col matrix's contract."""
    if not conv3s2_supported(t, B, H, W, C, ld, image=image):
        form = "image" if image else "token-major"
        raise _lib.VitmiError(f"{who}: unsupported ({form} form needs bf16 or fp32, C {'== 3' if image else 'a multiple of 8'}, "
                              f"ld a multiple of 8 and at least 9*C; got {t.dtype}, B {B}, H {H}, W {W}, C {C}, ld {ld})")
    M = B * ((H + 1) // 2) * ((W + 1) // 2)
    _contract(who, "col", t, t.dtype, M * ld, f"[B*Ho*Wo, ld] = [{M}, {ld}]")
    return M


def conv3s2_im2col(x, col, B, H, W, C):
    """col [B*ceil(H/2)*ceil(W/2), ld] (bf16 or fp32) = the 3x3 / stride 2 / padding 1 windows of x, k = c*9 + i*3 + j, the
    columns [9*C, ld) zero (vitmi_conv3s2_im2col).  x: the fp32 image [B, 3, H, W] in any strides (contiguous or
    channels_last), or the token-major activation [B, H*W, C] in col's dtype with C a multiple of 8."""
    _need_cuda(x, col)
    image = x.dim() == 4
    if col.dim() != 2:
        raise _lib.VitmiError(f"conv3s2_im2col: col must be a 2-d [rows, ld] tensor, got {tuple(col.shape)}")
    ld = col.shape[1]
    _conv3s2_check("conv3s2_im2col", col, B, H, W, C, ld, image)
    if image:
        if x.dtype != torch.float32 or tuple(x.shape) != (B, C, H, W):
            raise _lib.VitmiError(f"conv3s2_im2col: the image must be fp32 [B, C, H, W] = [{B}, {C}, {H}, {W}] "
                                  f"(got {x.dtype}, {tuple(x.shape)})")
        strides = x.stride()
    else:
        _contract("conv3s2_im2col", "x", x, col.dtype, B * H * W * C, f"[B, H*W, C] = [{B}, {H * W}, {C}]")
        strides = (0, 0, 0, 0)
    check(load().vitmi_conv3s2_im2col(x.data_ptr(), int(image), *strides, col.data_ptr(), dtype_code(col), ld, B, H, W, C,
                                      _stream()), "vitmi_conv3s2_im2col")
    return col


def conv3s2_col2im(dcol, dx, B, H, W, C):
    """dx [B, H*W, C] = the transpose of conv3s2_im2col's token-major form applied to dcol [B*Ho*Wo, ld]: each pixel sums,
    in fp32 in a fixed order, the 1, 2 or 4 entries that read it (vitmi_conv3s2_col2im; no atomics)."""
    _need_cuda(dcol, dx)
    if dcol.dim() != 2:
        raise _lib.VitmiError(f"conv3s2_col2im: dcol must be a 2-d [rows, ld] tensor, got {tuple(dcol.shape)}")
    ld = dcol.shape[1]
    _conv3s2_check("conv3s2_col2im", dcol, B, H, W, C, ld, False)
    _contract("conv3s2_col2im", "dx", dx, dcol.dtype, B * H * W * C, f"[B, H*W, C] = [{B}, {H * W}, {C}]")
    check(load().vitmi_conv3s2_col2im(dcol.data_ptr(), ld, dx.data_ptr(), dtype_code(dcol), B, H, W, C, _stream()),
          "vitmi_conv3s2_col2im")
    return dx


def conv3s2_wcopy(src, dst, cols):
    """dst[r, c] = src[r, c] for c < cols, 0 for the rest of dst's columns; src [rows, >= cols], dst [rows, >= cols], the same
    dtype (vitmi_conv3s2_wcopy): the K = 27 weight of the first stage to its [Cout, 32] image, and its gradient back."""
    _need_cuda(src, dst)
    if (src.dim() != 2 or dst.dim() != 2 or src.dtype != dst.dtype or src.dtype not in (torch.bfloat16, torch.float32)
            or src.shape[0] != dst.shape[0] or src.stride(1) != 1 or dst.stride(1) != 1 or cols > src.shape[1]
            or cols > dst.shape[1]):
        raise _lib.VitmiError(f"conv3s2_wcopy: src and dst must be 2-d bf16 or fp32 tensors of one dtype and row count with "
                              f"at least {cols} columns (got {src.dtype} {tuple(src.shape)}, {dst.dtype} {tuple(dst.shape)})")
    check(load().vitmi_conv3s2_wcopy(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), dtype_code(src),
                                     src.shape[0], cols, dst.shape[1], _stream()), "vitmi_conv3s2_wcopy")
    return dst


def bn_act_supported(t, M, C) -> bool:
    """Host-only query: do bn_act_fwd / bn_act_bwd take this dtype and shape?"""
    return bool(load().vitmi_bn_act_supported(dtype_code_or_neg(t), M, C))


def _bn_act_contract(who, y, acts, f32s, M, C):
    if y.dtype not in (torch.bfloat16, torch.float32):
        raise _lib.VitmiError(f"{who}: y must be bf16 or fp32, got {y.dtype}")
    for name, t in acts:
        _contract(who, name, t, y.dtype, M * C, f"[M, C] = [{M}, {C}]")
    for name, t, n in f32s:
        if t is not None:
            _contract(who, name, t, torch.float32, n, f"{n}-element")


def bn_act_fwd(y, gamma, beta, running_mean, running_var, num_batches_tracked, stat, out, M, C, *, gelu, training,
               momentum=0.1, eps=1e-5):
    """out [M, C] = act(BatchNorm(y)) over the rows of y [M, C] (bf16 or fp32) as stored; act = GELU (erf) if `gelu`, else
    nothing.  Writes stat fp32 [2, C] (mean, rstd), which bn_act_bwd needs.  training: batch statistics, and the three
    running buffers (fp32 [C], fp32 [C], int64 [1]; each may be None) are updated on the device; otherwise the running
    statistics are used and nothing is touched (vitmi_bn_act_fwd)."""
    _need_cuda(y, gamma, beta, running_mean, running_var, num_batches_tracked, stat, out)
    _bn_act_contract("bn_act_fwd", y, (("y", y), ("out", out)),
                     (("weight", gamma, C), ("bias", beta, C), ("stat", stat, 2 * C), ("running_mean", running_mean, C),
                      ("running_var", running_var, C)), M, C)
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1):
        raise _lib.VitmiError("bn_act_fwd: num_batches_tracked must be an int64 tensor of one element")
    if not training and (running_mean is None or running_var is None):
        raise _lib.VitmiError("bn_act_fwd: eval mode needs running_mean and running_var")
    code = dtype_code(y)
    ptr, nb = _aligned_ws(load().vitmi_bn_act_workspace(code, M, C), y.device)
    check(load().vitmi_bn_act_fwd(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean), _ptr(running_var),
                                  _ptr(num_batches_tracked), stat.data_ptr(), out.data_ptr(), code, int(bool(gelu)),
                                  int(bool(training)), momentum, eps, M, C, ptr, nb, _stream()), "vitmi_bn_act_fwd")
    return out


def bn_act_bwd(dout, y, stat, gamma, beta, dy, dgamma, dbeta, M, C, *, gelu, training):
    """Backward of bn_act_fwd: dy (compute dtype, not aliasing dout) and the fp32 dgamma, dbeta, stored, from dout, the
    stored y and stat (vitmi_bn_act_bwd); training=False is the eval-mode gradient."""
    _need_cuda(dout, y, stat, gamma, beta, dy, dgamma, dbeta)
    _bn_act_contract("bn_act_bwd", y, (("y", y), ("dout", dout), ("dy", dy)),
                     (("stat", stat, 2 * C), ("weight", gamma, C), ("bias", beta, C), ("dgamma", dgamma, C),
                      ("dbeta", dbeta, C)), M, C)
    if dy.data_ptr() == dout.data_ptr():
        raise _lib.VitmiError("bn_act_bwd: dy must not alias dout")
    code = dtype_code(y)
    ptr, nb = _aligned_ws(load().vitmi_bn_act_workspace(code, M, C), y.device)
    check(load().vitmi_bn_act_bwd(dout.data_ptr(), y.data_ptr(), stat.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                  dy.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), code, int(bool(gelu)),
                                  int(bool(training)), M, C, ptr, nb, _stream()), "vitmi_bn_act_bwd")
    return dy


def posfourier_supported(t, Hp, Wp, hidden_dim) -> bool:
    """Host-only query: does posfourier_features build this table (bf16 or fp32, hidden_dim 32)?"""
    return bool(load().vitmi_posfourier_supported(dtype_code_or_neg(t), Hp, Wp, hidden_dim))


def posfourier_features(out, Hp, Wp, hidden_dim=32, temperature=10000.0):
    """out [Hp*Wp, 2*hidden_dim] (bf16 or fp32) = the sin / cos feature table of XCiT's PositionalEncodingFourier before its
    1x1 projection: hidden_dim y-features then hidden_dim x-features, sin at even and cos at odd indices, for one image
    (vitmi_posfourier_features).  hidden_dim must be 32."""
    _need_cuda(out)
    if not posfourier_supported(out, Hp, Wp, hidden_dim):
        raise _lib.VitmiError(f"posfourier_features: unsupported (needs bf16 or fp32, hidden_dim 32, a grid of at least 1 x 1; "
                              f"got {out.dtype}, hidden_dim {hidden_dim}, grid {Hp} x {Wp})")
    _contract("posfourier_features", "out", out, out.dtype, Hp * Wp * 2 * hidden_dim,
              f"[Hp*Wp, 2*hidden_dim] = [{Hp * Wp}, {2 * hidden_dim}]")
    check(load().vitmi_posfourier_features(out.data_ptr(), dtype_code(out), Hp, Wp, hidden_dim, float(temperature), _stream()),
          "vitmi_posfourier_features")
    return out


def add_rows_bcast_supported(t, B, N, C) -> bool:
    """Host-only query: does add_rows_bcast take this dtype and shape?"""
    return bool(load().vitmi_add_rows_bcast_supported(dtype_code_or_neg(t), B, N, C))


def add_rows_bcast(x, pos, out, B, N, C):
    """out[b, n, :] = x[b, n, :] + pos[n, :]: x, out [B, N, C] in one dtype (bf16 or fp32), pos fp32 [N, C]
    (vitmi_add_rows_bcast)."""
    _need_cuda(x, pos, out)
    if not add_rows_bcast_supported(x, B, N, C):
        raise _lib.VitmiError(f"add_rows_bcast: unsupported (needs bf16 or fp32 and B, N, C >= 1; got {x.dtype}, B {B}, N {N}, C {C})")
    _contract("add_rows_bcast", "x", x, x.dtype, B * N * C, f"[B, N, C] = [{B}, {N}, {C}]")
    _contract("add_rows_bcast", "out", out, x.dtype, B * N * C, f"[B, N, C] = [{B}, {N}, {C}]")
    _contract("add_rows_bcast", "pos", pos, torch.float32, N * C, f"[N, C] = [{N}, {C}]")
    check(load().vitmi_add_rows_bcast(x.data_ptr(), pos.data_ptr(), out.data_ptr(), dtype_code(x), B, N, C, _stream()),
          "vitmi_add_rows_bcast")
    return out


def ca_glue_supported(t, B, N1, D) -> bool:
    """Host-only query: do ca_merge_fwd / ca_merge_bwd / ca_out_fwd / ca_out_bwd take this operand dtype and shape?"""
    return bool(load().vitmi_ca_glue_supported(dtype_code_or_neg(t), B, N1, D))


def _ca_contract(who, op, B, N1, D, res=(), rows=(), cls=(), vecs=()):
    """The class-attention glue's contracts: `op` (a [B, D] operand) fixes the operand dtype; `res` (name, tensor) are fp32
    [B, N1, D]; `rows` operand-dtype [B, N1, D]; `cls` operand-dtype [B, D]; `vecs` fp32 [D]."""
    if not ca_glue_supported(op, B, N1, D):
        raise _lib.VitmiError(f"{who}: unsupported (needs bf16 or fp32 operands, N1 >= 2 and D a multiple of 8; got {op.dtype}, "
                              f"B {B}, N1 {N1}, D {D})")
    for name, t in res:
        _contract(who, name, t, torch.float32, B * N1 * D, f"[B, N1, D] = [{B}, {N1}, {D}]")
    for name, t in rows:
        _contract(who, name, t, op.dtype, B * N1 * D, f"[B, N1, D] = [{B}, {N1}, {D}]")
    for name, t in cls:
        _contract(who, name, t, op.dtype, B * D, f"[B, D] = [{B}, {D}]")
    for name, t in vecs:
        _contract(who, name, t, torch.float32, D, f"[D] = [{D}]")


def ca_merge_fwd(x, a, l, gamma1, x1, B, N1, D):
    """x1[b, n, :] = x[b, n, :] + gamma1 * (n == 0 ? a[b, :] : l[b, n, :]): the first residual of XCiT's class-attention
    block, whose attention returns cat[proj(cls), norm1(x)[:, 1:]].  x, x1 fp32; a [B, D], l [B, N1, D] bf16 or fp32."""
    _need_cuda(x, a, l, gamma1, x1)
    _ca_contract("ca_merge_fwd", a, B, N1, D, res=(("x", x), ("x1", x1)), rows=(("l", l),), cls=(("a", a),),
                 vecs=(("gamma1", gamma1),))
    check(load().vitmi_ca_merge_fwd(x.data_ptr(), a.data_ptr(), l.data_ptr(), gamma1.data_ptr(), x1.data_ptr(), dtype_code(a),
                                    B, N1, D, _stream()), "vitmi_ca_merge_fwd")
    return x1


def ca_merge_bwd(dx1, l, a, gamma1, da, dl, dgamma1, B, N1, D):
    """Backward of ca_merge_fwd's branch: da [B, D] = gamma1 * dx1[:, 0] (operand dtype); dl fp32 [B, N1, D] = gamma1 *
    dx1 on the patch rows and 0 on the CLS rows (stored: accumulate the projections' data gradients onto it); dgamma1 fp32
    [D], stored, summed over every row against a (row 0) or l (the rest) in two levels without atomics."""
    _need_cuda(dx1, l, a, gamma1, da, dl, dgamma1)
    _ca_contract("ca_merge_bwd", a, B, N1, D, res=(("dx1", dx1), ("dl", dl)), rows=(("l", l),), cls=(("a", a), ("da", da)),
                 vecs=(("gamma1", gamma1), ("dgamma1", dgamma1)))
    ptr, nb = _aligned_ws(load().vitmi_ca_merge_bwd_workspace(B, N1, D), dx1.device)
    check(load().vitmi_ca_merge_bwd(dx1.data_ptr(), l.data_ptr(), a.data_ptr(), gamma1.data_ptr(), da.data_ptr(), dl.data_ptr(),
                                    dgamma1.data_ptr(), dtype_code(a), B, N1, D, ptr, nb, _stream()), "vitmi_ca_merge_bwd")
    return dl


def ca_out_fwd(xc, xp, m, gamma2, out, B, N1, D):
    """out[b, n, :] = n == 0 ? xc[b, :] + gamma2 * m[b, :] : 2 * xp[b, n, :]: the block's last line, x_res + cat[gamma2 *
    mlp(cls), x[:, 1:]].  xc: the normed CLS rows, an fp32 [B, D] tensor or view with unit column stride (row 0 of each
    image of norm2's output, or its compact output); xp fp32 [B, N1, D] holds the patch rows; m [B, D] bf16 or fp32."""
    _need_cuda(xc, xp, m, gamma2, out)
    _ca_contract("ca_out_fwd", m, B, N1, D, res=(("xp", xp), ("out", out)), cls=(("m", m),), vecs=(("gamma2", gamma2),))
    if xc.dtype != torch.float32 or tuple(xc.shape) != (B, D) or xc.stride(1) != 1:
        raise _lib.VitmiError(f"ca_out_fwd: xc must be an fp32 [B, D] = [{B}, {D}] tensor or row view (got {xc.dtype}, "
                              f"{tuple(xc.shape)}, strides {xc.stride()})")
    check(load().vitmi_ca_out_fwd(xc.data_ptr(), xc.stride(0) if B > 1 else D, xp.data_ptr(), m.data_ptr(), gamma2.data_ptr(),
                                  out.data_ptr(), dtype_code(m), B, N1, D, _stream()), "vitmi_ca_out_fwd")
    return out


def ca_out_bwd(G, gamma2, dx2, gm, B, N1, D):
    """Backward of ca_out_fwd without the MLP: dx2[b, n, :] = n == 0 ? G[b, 0, :] : 2 * G[b, n, :] (fp32) and gm [B, D] =
    gamma2 * G[:, 0] in the operand dtype (gm's), the gradient that enters the MLP."""
    _need_cuda(G, gamma2, dx2, gm)
    _ca_contract("ca_out_bwd", gm, B, N1, D, res=(("G", G), ("dx2", dx2)), cls=(("gm", gm),), vecs=(("gamma2", gamma2),))
    check(load().vitmi_ca_out_bwd(G.data_ptr(), gamma2.data_ptr(), dx2.data_ptr(), gm.data_ptr(), dtype_code(gm), B, N1, D,
                                  _stream()), "vitmi_ca_out_bwd")
    return dx2


def ls_residual_ln_supported(t, M, D) -> bool:
    """Host-only query: does ls_residual_ln_fwd take this branch dtype and shape (D a multiple of 8, 8 <= D <= 2048)?"""
    return bool(load().vitmi_ls_residual_ln_supported(dtype_code_or_neg(t), M, D))


def ls_residual_ln_fwd(x, b, gamma, ln_weight, ln_bias, y, l, mean, rstd, eps, *, M=None, D=None):
    """y = x + gamma * b and l = LayerNorm(y) in one pass (vitmi_ls_residual_ln_fwd, layernorm.hip): the junction of a LayerScale
    residual branch that does not end in a GEMM and the norm that reads the sum.  x, y fp32 [M, D] (y may be x); b, l [M, D] in one
    dtype, bf16 or fp32; gamma, ln_weight, ln_bias fp32 [D]; mean, rstd fp32 [M], of y."""
    _need_cuda(x, b, gamma, ln_weight, ln_bias, y, l, mean, rstd)
    D = D or x.shape[-1]
    M = M or x.numel() // D
    if not ls_residual_ln_supported(b, M, D):
        raise _lib.VitmiError(f"ls_residual_ln_fwd: unsupported (needs bf16 or fp32 b / l, M >= 1 and D a multiple of 8 with "
                              f"8 <= D <= 2048; got {b.dtype}, M {M}, D {D})")
    for name, t in (("x", x), ("y", y)):
        _contract("ls_residual_ln_fwd", name, t, torch.float32, M * D, f"[M, D] = [{M}, {D}]")
    for name, t in (("b", b), ("l", l)):
        _contract("ls_residual_ln_fwd", name, t, b.dtype, M * D, f"[M, D] = [{M}, {D}]")
    for name, t in (("gamma", gamma), ("ln_weight", ln_weight), ("ln_bias", ln_bias)):
        _contract("ls_residual_ln_fwd", name, t, torch.float32, D, f"[D] = [{D}]")
    for name, t in (("mean", mean), ("rstd", rstd)):
        _contract("ls_residual_ln_fwd", name, t, torch.float32, M, f"[M] = [{M}]")
    check(load().vitmi_ls_residual_ln_fwd(x.data_ptr(), b.data_ptr(), gamma.data_ptr(), ln_weight.data_ptr(), ln_bias.data_ptr(),
                                          y.data_ptr(), l.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dtype_code(b), M, D,
                                          float(eps), _stream()), "vitmi_ls_residual_ln_fwd")
    return y


def attn_bwd_dbias_rows(B, N) -> int:
    return int(load().vitmi_attn_bwd_dbias_rows(B, N))


def attn_bwd(qkv, out, dout, lse, dqkv, B, N, H, hd, scale, dbias_part=None, launch_flags=0):
    """dbias_part (bf16 only): fp32 [attn_bwd_dbias_rows(B, N), 3*H*hd] partial column sums of dqkv."""
    _need_cuda(qkv, out, dout, dqkv)
    assert qkv.is_contiguous() and out.is_contiguous() and dout.is_contiguous() and dqkv.is_contiguous()
    lib = load()
    if dbias_part is not None:
        assert dbias_part.dtype == torch.float32 and dbias_part.is_contiguous()
        assert tuple(dbias_part.shape) == (attn_bwd_dbias_rows(B, N), 3 * H * hd)
    ws = workspace(lib.vitmi_attn_bwd_workspace(B, N, H), qkv.device)
    check(lib.vitmi_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                             dqkv.data_ptr(), dtype_code(qkv), B, N, H, hd, float(scale), _ptr(dbias_part),
                             int(launch_flags), ws.data_ptr(), ws.numel(), _stream()), "vitmi_attn_bwd")
    return dqkv


def cast(src, dst):
    _need_cuda(src, dst)
    assert src.numel() == dst.numel() and src.is_contiguous() and dst.is_contiguous()
    check(load().vitmi_cast(src.data_ptr(), dtype_code(src), dst.data_ptr(), dtype_code(dst),
                            src.numel(), _stream()), "vitmi_cast")
    return dst


def axpy(x, y, a=1.0):
    """y += a * x (fp32, contiguous): gradient accumulation over a span of the flat gradient buffer."""
    _need_cuda(x, y)
    assert x.dtype == y.dtype == torch.float32 and x.numel() == y.numel() and x.is_contiguous() and y.is_contiguous()
    check(load().vitmi_axpy(x.data_ptr(), y.data_ptr(), float(a), x.numel(), _stream()), "vitmi_axpy")
    return y


def patchify(x, out, p, cls_rows):
    """x [B,C,H,W] fp32 (any strides) -> out [B*(cls_rows+gh*gw), ld] with ld >= C*p*p; the columns
    beyond C*p*p are written as zeros (K padding for the tile GEMM)."""
    _need_cuda(x, out)
    assert x.dtype == torch.float32 and x.dim() == 4 and out.dim() == 2 and out.is_contiguous()
    B, Cc, H, W = x.shape
    assert out.shape[1] >= Cc * p * p and out.shape[1] % 4 == 0
    sb, sc, sh, sw = x.stride()
    check(load().vitmi_patchify(x.data_ptr(), sb, sc, sh, sw, out.data_ptr(), dtype_code(out), out.shape[1],
                                B, Cc, H, W, p, int(cls_rows), _stream()), "vitmi_patchify")
    return out


def pos_resample(src, table, out=None):
    """out[r] = sum_e w[e] * src[col[e]] over row r's entries of `table` = (row_ptr, col, w, rows):
    the bicubic pos_embed resize, or with the transposed table its backward (posembed.py)."""
    row_ptr, col, w, rows = table
    _need_cuda(src, row_ptr, col, w)
    assert src.dtype == torch.float32 and src.dim() == 2 and src.stride(1) == 1
    assert row_ptr.dtype == torch.int32 and col.dtype == torch.int32 and w.dtype == torch.float32
    assert row_ptr.numel() == rows + 1
    D = src.shape[1]
    if out is None:
        out = torch.empty((rows, D), dtype=torch.float32, device=src.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (rows, D) and out.stride(1) == 1
    check(load().vitmi_pos_resample(src.data_ptr(), src.stride(0), row_ptr.data_ptr(), col.data_ptr(), w.data_ptr(),
                                    out.data_ptr(), out.stride(0), rows, D, _stream()), "vitmi_pos_resample")
    return out


FOLD_DIRECT_ROWS = 2048      # vitmi_colsum folds an fp32 matrix of at most this many rows in one reduce_rows launch


def colsum(x, out, *, M=None, N=None, ld=None, fold=None):
    """fold (a FoldQueue): a short fp32 matrix (a partial buffer) is queued instead of folded now — the same sum."""
    _need_cuda(x, out)
    N = N or x.shape[-1]
    M = M or x.numel() // N
    ld = ld or N
    assert out.dtype == torch.float32 and out.numel() >= N
    if fold is not None and x.dtype == torch.float32 and M <= FOLD_DIRECT_ROWS:
        fold.add(x, M, N, ld, [out])
        return out
    lib = load()
    ws = workspace(lib.vitmi_colsum_workspace(M, N), x.device)
    check(lib.vitmi_colsum(x.data_ptr(), dtype_code(x), M, N, ld, out.data_ptr(), ws.data_ptr(),
                           ws.numel(), _stream()), "vitmi_colsum")
    return out


def softmax_xent(logits, labels, loss_buf, dlogits, correct_buf):
    """loss_buf fp32 [1+B] (loss_buf[0] = mean loss), correct_buf int32 [1+B]."""
    _need_cuda(logits, labels, loss_buf, dlogits, correct_buf)
    B, K = logits.shape
    assert logits.dtype == torch.float32 and logits.is_contiguous() and labels.dtype == torch.int64
    assert loss_buf.numel() >= 1 + B and correct_buf.numel() >= 1 + B and correct_buf.dtype == torch.int32
    check(load().vitmi_softmax_xent(logits.data_ptr(), labels.data_ptr(), loss_buf.data_ptr(),
                                    dlogits.data_ptr(), correct_buf.data_ptr(), B, K, _stream()),
          "vitmi_softmax_xent")


def sgd_momentum(p, g, buf, shadow, lr, momentum, grad_scale=1.0):
    _need_cuda(p, g, buf)
    assert p.dtype == g.dtype == buf.dtype == torch.float32
    assert p.numel() == g.numel() == buf.numel()
    check(load().vitmi_sgd_momentum(p.data_ptr(), g.data_ptr(), buf.data_ptr(), _ptr(shadow),
                                    p.numel(), float(lr), float(momentum), float(grad_scale),
                                    _stream()), "vitmi_sgd_momentum")


def _ingest_args(src, dst, off_y, off_x, flip, mean, std):
    """What the four ingest wrappers ask of their arguments: a contiguous uint8 [B,H,W,C] (NHWC) source, a contiguous
    destination, and the five optional tensors (crop offsets, flip flags, channel mean / std) contiguous, on the GPU and of
    their dtype.  Returns the source's shape."""
    _need_cuda(src, dst)
    assert src.dtype == torch.uint8 and src.is_contiguous() and dst.is_contiguous()
    for t, dt in ((off_y, torch.int32), (off_x, torch.int32), (flip, torch.uint8), (mean, torch.float32), (std, torch.float32)):
        assert t is None or (t.is_cuda and t.dtype == dt and t.is_contiguous())
    return src.shape


def image_ingest(src, dst, off_y, off_x, flip, mean, std, pad, fill=128):
    """src uint8 [B,H,W,C] (NHWC) -> dst fp32 [B,C,S,S]; see vitmi_image_ingest."""
    B, H, W, C = _ingest_args(src, dst, off_y, off_x, flip, mean, std)
    assert dst.dtype == torch.float32 and dst.shape[0] == B and dst.shape[1] == C and dst.shape[2] == dst.shape[3]
    check(load().vitmi_image_ingest(src.data_ptr(), dst.data_ptr(), _ptr(off_y), _ptr(off_x), _ptr(flip), _ptr(mean),
                                    _ptr(std), B, H, W, C, dst.shape[2], int(pad), int(fill), _stream()),
          "vitmi_image_ingest")
    return dst


def ingest_patchify(src, out, off_y, off_x, flip, mean, std, S, pad, p, cls_rows, fill=128):
    """src uint8 [B,H,W,C] (NHWC) -> out [B*(cls_rows + (S/p)^2), ld >= C*p*p] patch rows; see vitmi_ingest_patchify."""
    B, H, W, C = _ingest_args(src, out, off_y, off_x, flip, mean, std)
    assert out.dim() == 2 and out.shape[0] == B * (cls_rows + (S // p) ** 2) and out.shape[1] >= C * p * p
    check(load().vitmi_ingest_patchify(src.data_ptr(), out.data_ptr(), dtype_code(out), out.shape[1], _ptr(off_y), _ptr(off_x),
                                       _ptr(flip), _ptr(mean), _ptr(std), B, H, W, C, int(S), int(pad), int(fill), int(p),
                                       int(cls_rows), _stream()), "vitmi_ingest_patchify")
    return out


def _resize_tables(ytab, xtab):
    for t in (ytab, xtab):
        assert t.is_cuda and t.dtype == torch.int32 and t.dim() == 2 and t.shape[0] >= 3 and t.is_contiguous()
    return ytab.data_ptr(), ytab.shape[0] - 2, ytab.shape[1], xtab.data_ptr(), xtab.shape[0] - 2, xtab.shape[1]


def resize_ingest(src, dst, ytab, xtab, off_y, off_x, flip, mean, std, pad, fill=128):
    """src uint8 [B,H,W,C] (NHWC) -> Pillow bicubic to ytab.shape[1] x xtab.shape[1] -> crop/flip/normalize -> dst fp32
    [B,C,S,S]; tables from vit_torch_amd.resize.table.  See vitmi_resize_ingest."""
    B, H, W, C = _ingest_args(src, dst, off_y, off_x, flip, mean, std)
    assert dst.dtype == torch.float32 and dst.shape[0] == B and dst.shape[1] == C and dst.shape[2] == dst.shape[3]
    check(load().vitmi_resize_ingest(src.data_ptr(), dst.data_ptr(), *_resize_tables(ytab, xtab), _ptr(off_y), _ptr(off_x),
                                     _ptr(flip), _ptr(mean), _ptr(std), B, H, W, C, dst.shape[2], int(pad), int(fill),
                                     _stream()), "vitmi_resize_ingest")
    return dst


def resize_ingest_patchify(src, out, ytab, xtab, off_y, off_x, flip, mean, std, S, pad, p, cls_rows, fill=128):
    """resize_ingest written straight into patch rows [B*(cls_rows + (S/p)^2), ld >= C*p*p]; see
    vitmi_resize_ingest_patchify."""
    B, H, W, C = _ingest_args(src, out, off_y, off_x, flip, mean, std)
    assert out.dim() == 2 and out.shape[0] == B * (cls_rows + (S // p) ** 2) and out.shape[1] >= C * p * p
    check(load().vitmi_resize_ingest_patchify(src.data_ptr(), out.data_ptr(), dtype_code(out), out.shape[1],
                                              *_resize_tables(ytab, xtab), _ptr(off_y), _ptr(off_x), _ptr(flip), _ptr(mean),
                                              _ptr(std), B, H, W, C, int(S), int(pad), int(fill), int(p), int(cls_rows),
                                              _stream()), "vitmi_resize_ingest_patchify")
    return out


def resize_ingest_plan(H, W, C, Hr, Wr, ytaps, xtaps, S, pad, fill=128, band_unit=1):
    """(band_rows, lds_bytes) a resize_ingest (band_unit 1) or resize_ingest_patchify (band_unit p) launch of this
    geometry runs with; raises where the launch would refuse it.  Host arithmetic only: see vitmi_resize_ingest_plan."""
    ct = _lib.C                                                           # the module's C is the channel count here
    band_rows, lds_bytes = ct.c_int(0), ct.c_int64(0)
    check(load().vitmi_resize_ingest_plan(int(H), int(W), int(C), int(Hr), int(Wr), int(ytaps), int(xtaps), int(S), int(pad),
                                          int(fill), int(band_unit), ct.byref(band_rows), ct.byref(lds_bytes)),
          "vitmi_resize_ingest_plan")
    return band_rows.value, lds_bytes.value


def adam(p, g, m, v, shadow, state, lr, beta1, beta2, eps, weight_decay, decoupled, grad_scale=1.0):
    _need_cuda(p, g, m, v, state)
    assert p.dtype == g.dtype == m.dtype == v.dtype == state.dtype == torch.float32
    assert p.numel() == g.numel() == m.numel() == v.numel() and state.numel() >= 1
    check(load().vitmi_adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(shadow), state.data_ptr(),
                            p.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                            int(bool(decoupled)), float(grad_scale), _stream()), "vitmi_adam")


def adagrad(p, g, acc, shadow, state, lr, lr_decay, eps, weight_decay, grad_scale=1.0):
    _need_cuda(p, g, acc, state)
    assert p.dtype == g.dtype == acc.dtype == state.dtype == torch.float32 and p.numel() == g.numel() == acc.numel()
    check(load().vitmi_adagrad(p.data_ptr(), g.data_ptr(), acc.data_ptr(), _ptr(shadow), state.data_ptr(), p.numel(),
                               float(lr), float(lr_decay), float(eps), float(weight_decay), float(grad_scale),
                               _stream()), "vitmi_adagrad")


def adadelta(p, g, square_avg, acc_delta, shadow, lr, rho, eps, weight_decay, grad_scale=1.0):
    _need_cuda(p, g, square_avg, acc_delta)
    assert p.dtype == g.dtype == square_avg.dtype == acc_delta.dtype == torch.float32
    assert p.numel() == g.numel() == square_avg.numel() == acc_delta.numel()
    check(load().vitmi_adadelta(p.data_ptr(), g.data_ptr(), square_avg.data_ptr(), acc_delta.data_ptr(), _ptr(shadow),
                                p.numel(), float(lr), float(rho), float(eps), float(weight_decay), float(grad_scale),
                                _stream()), "vitmi_adadelta")


def adabelief(p, g, m, s, shadow, state, lr, beta1, beta2, eps, weight_decay, decoupled, rectify, grad_scale=1.0):
    _need_cuda(p, g, m, s, state)
    assert p.dtype == g.dtype == m.dtype == s.dtype == state.dtype == torch.float32
    assert p.numel() == g.numel() == m.numel() == s.numel()
    check(load().vitmi_adabelief(p.data_ptr(), g.data_ptr(), m.data_ptr(), s.data_ptr(), _ptr(shadow), state.data_ptr(),
                                 p.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                 int(bool(decoupled)), int(bool(rectify)), float(grad_scale), _stream()), "vitmi_adabelief")


# ------------------------------------------------------------------ CaiT ops ---
def th_softmax_fwd(S, Wl, bl, Ww, bw, P, Pm, B, H, N, Nk, ld):
    _need_cuda(S, P, Pm)
    check(load().vitmi_th_softmax_fwd(S.data_ptr(), Wl.data_ptr(), bl.data_ptr(), Ww.data_ptr(), bw.data_ptr(),
                                      P.data_ptr(), Pm.data_ptr(), dtype_code(S), B, H, N, Nk, ld, _stream()),
          "vitmi_th_softmax_fwd")


def th_softmax_bwd(S, P, dPm, Wl, Ww, dS, dWl, dbl, dWw, dbw, B, H, N, Nk, ld):
    _need_cuda(S, P, dPm, dS)
    lib = load()
    ws = workspace(lib.vitmi_th_softmax_bwd_workspace(B, H, N), S.device)
    check(lib.vitmi_th_softmax_bwd(S.data_ptr(), P.data_ptr(), dPm.data_ptr(), Wl.data_ptr(), Ww.data_ptr(),
                                   dS.data_ptr(), dWl.data_ptr(), dbl.data_ptr(), dWw.data_ptr(), dbw.data_ptr(),
                                   dtype_code(S), B, H, N, Nk, ld, ws.data_ptr(), ws.numel(), _stream()),
          "vitmi_th_softmax_bwd")


TH_LONG_MAXH, TH_LONG_MAXN = 16, 1024      # th_softmax_fwd / _bwd limits (cait_ops.hip TH_LONG_MAXH / TH_LONG_MAXC)


def th_scores_softmax(qkv, Wl, bl, Ww, bw, B, H, N, hd, scale, NS):
    """The first two of the three calls: S = scale q k^T into [B,H,N,NS] score rows, then the talking-heads softmax.
    Returns (S, P, Pm)."""
    D, D3 = H * hd, 3 * H * hd
    S = torch.empty((B, H, N, NS), dtype=qkv.dtype, device=qkv.device)
    gemm_batched(qkv, qkv, S, M=N, N=N, K=hd, lda=D3, ldb=D3, ldc=NS, a_kmajor=True, b_kmajor=True,
                 batch=B * H, batch_inner=H, a_bs=(N * D3, hd), b_bs=(N * D3, hd),
                 c_bs=(H * N * NS, N * NS), b_off=D, alpha=scale)
    P, Pm = torch.empty_like(S), torch.empty_like(S)
    th_softmax_fwd(S, Wl, bl, Ww, bw, P, Pm, B, H, N, N, NS)
    return S, P, Pm


def th_three_call_fwd(qkv, Wl, bl, Ww, bw, O, B, H, N, hd, scale, NS):
    """Talking-heads attention in three calls: th_scores_softmax, then O [B*N, H*hd] = P' v.  Returns (S, P, Pm) for
    th_three_call_bwd."""
    D, D3 = H * hd, 3 * H * hd
    S, P, Pm = th_scores_softmax(qkv, Wl, bl, Ww, bw, B, H, N, hd, scale, NS)
    gemm_batched(Pm, qkv, O, M=N, N=hd, K=N, lda=NS, ldb=D3, ldc=D, a_kmajor=True, b_kmajor=False,
                 batch=B * H, batch_inner=H, a_bs=(H * N * NS, N * NS), b_bs=(N * D3, hd),
                 c_bs=(N * D, hd), b_off=2 * D)
    return S, P, Pm


def th_three_call_bwd(qkv, dO, S, P, Pm, Wl, Ww, dqkv, dWl, dbl, dWw, dbw, B, H, N, hd, scale, NS):
    """Backward of th_three_call_fwd: dq, dk, dv into dqkv [B*N, 3*H*hd] and the four mixing-parameter gradients.
    The transients dP' and dS are dropped as soon as their last product has been queued."""
    D, D3 = H * hd, 3 * H * hd
    dPm = torch.empty_like(S)
    gemm_batched(dO, qkv, dPm, M=N, N=N, K=hd, lda=D, ldb=D3, ldc=NS, a_kmajor=True, b_kmajor=True,
                 batch=B * H, batch_inner=H, a_bs=(N * D, hd), b_bs=(N * D3, hd),
                 c_bs=(H * N * NS, N * NS), b_off=2 * D)
    dS = torch.empty_like(S)
    th_softmax_bwd(S, P, dPm, Wl, Ww, dS, dWl, dbl, dWw, dbw, B, H, N, N, NS)
    del dPm
    gemm_batched(dS, qkv, dqkv, M=N, N=hd, K=N, lda=NS, ldb=D3, ldc=D3, a_kmajor=True, b_kmajor=False,
                 batch=B * H, batch_inner=H, a_bs=(H * N * NS, N * NS), b_bs=(N * D3, hd),
                 c_bs=(N * D3, hd), b_off=D, alpha=scale)                                  # dQ = scale dS K
    gemm_batched(Pm, dO, dqkv, M=N, N=hd, K=N, lda=NS, ldb=D, ldc=D3, a_kmajor=False, b_kmajor=False,
                 batch=B * H, batch_inner=H, a_bs=(H * N * NS, N * NS), b_bs=(N * D, hd),
                 c_bs=(N * D3, hd), c_off=2 * D)                                           # dV = P'^T dO
    gemm_batched(dS, qkv, dqkv, M=N, N=hd, K=N, lda=NS, ldb=D3, ldc=D3, a_kmajor=False, b_kmajor=False,
                 batch=B * H, batch_inner=H, a_bs=(H * N * NS, N * NS), b_bs=(N * D3, hd),
                 c_bs=(N * D3, hd), c_off=D, alpha=scale)                                  # dK = scale dS^T Q


def th_long_supported(t, H, N, hd) -> bool:
    """Host-only query: does the long-sequence talking-heads op (th_long_fwd / _bwd) take this shape / dtype?  bf16 only:
    the parity modes keep their scores (th_three_call_*); the limits are those of th_softmax_fwd / _bwd."""
    return t == torch.bfloat16 and 1 <= H <= TH_LONG_MAXH and 1 <= N <= TH_LONG_MAXN and hd >= 1


def _th_long_check(qkv, B, H, N, hd):
    if not th_long_supported(qkv.dtype, H, N, hd):
        raise _lib.VitmiError(f"th_long: bf16 with H <= {TH_LONG_MAXH} heads and N <= {TH_LONG_MAXN} tokens required "
                         f"(got {qkv.dtype}, H = {H}, N = {N}, hd = {hd})")
    assert qkv.is_contiguous() and qkv.numel() == B * N * 3 * H * hd


def th_long_fwd(qkv, Wl, bl, Ww, bw, O, B, H, N, hd, scale):
    """Talking-heads attention that keeps nothing quadratic: O [B*N, H*hd] as th_three_call_fwd computes it, with the
    score tensors dropped on return.  th_long_bwd recomputes them from qkv, one layer at a time."""
    _th_long_check(qkv, B, H, N, hd)
    th_three_call_fwd(qkv, Wl, bl, Ww, bw, O, B, H, N, hd, scale, (N + 7) // 8 * 8)
    return O


def th_long_bwd(qkv, dO, Wl, bl, Ww, bw, dqkv, dWl, dbl, dWw, dbw, B, H, N, hd, scale):
    """Backward of th_long_fwd: recomputes S, P and P' (not O) and runs the three-call backward.  Peak transient: five
    [B, H, N, ru8(N)] bf16 tensors (S, P, P', dP', dS) while the softmax backward runs, all freed before it returns."""
    _th_long_check(qkv, B, H, N, hd)
    NS = (N + 7) // 8 * 8
    S, P, Pm = th_scores_softmax(qkv, Wl, bl, Ww, bw, B, H, N, hd, scale, NS)
    th_three_call_bwd(qkv, dO, S, P, Pm, Wl, Ww, dqkv, dWl, dbl, dWw, dbw, B, H, N, hd, scale, NS)


def th_attn_supported(t, H, N, hd) -> bool:
    """Host-only query: do the fused talking-heads kernels take this shape / dtype?"""
    return bool(load().vitmi_th_attn_supported(dtype_code_or_neg(t), H, N, hd))


def th_attn_fwd(qkv, Wl, bl, Ww, bw, out, B, H, N, hd, scale):
    """out [B,N,H,hd] = talking-heads attention of qkv [B,N,3,H,hd] (vitmi_th_attn_fwd: scores never leave the CU)."""
    _need_cuda(qkv, out)
    assert qkv.is_contiguous() and out.is_contiguous()
    ptr, nb = _aligned_ws(load().vitmi_th_attn_workspace(B, H, N, hd), qkv.device)
    check(load().vitmi_th_attn_fwd(qkv.data_ptr(), Wl.data_ptr(), bl.data_ptr(), Ww.data_ptr(), bw.data_ptr(), out.data_ptr(),
                                   dtype_code(qkv), B, H, N, hd, float(scale), ptr, nb, _stream()), "vitmi_th_attn_fwd")
    return out


def th_attn_bwd(qkv, dout, Wl, bl, Ww, bw, dqkv, dS, Pm, ld, dWl, dbl, dWw, dbw, B, H, N, hd, scale):
    """dQ into dqkv's q slots, dS and Pm ([B,H,N,ld]) for the caller's dK / dV products, the four mixing-parameter gradients."""
    _need_cuda(qkv, dout, dqkv, dS, Pm)
    assert qkv.is_contiguous() and dout.is_contiguous() and dqkv.is_contiguous() and dS.is_contiguous() and Pm.is_contiguous()
    ptr, nb = _aligned_ws(load().vitmi_th_attn_workspace(B, H, N, hd), qkv.device)
    check(load().vitmi_th_attn_bwd(qkv.data_ptr(), dout.data_ptr(), Wl.data_ptr(), bl.data_ptr(), Ww.data_ptr(), bw.data_ptr(),
                                   dqkv.data_ptr(), dS.data_ptr(), Pm.data_ptr(), ld, dWl.data_ptr(), dbl.data_ptr(), dWw.data_ptr(),
                                   dbw.data_ptr(), dtype_code(qkv), B, H, N, hd, float(scale), ptr, nb, _stream()), "vitmi_th_attn_bwd")


def class_attn_fwd(q, k, v, kv_stride, out, p_save, B, H, N, hd, scale):
    _need_cuda(q, k, v, out, p_save)
    check(load().vitmi_class_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), kv_stride, out.data_ptr(),
                                      p_save.data_ptr(), dtype_code(q), B, H, N, hd, float(scale), _stream()),
          "vitmi_class_attn_fwd")


def class_attn_bwd(q, k, v, kv_stride, dout, p_save, dq, dk, dv, dkv_stride, B, H, N, hd, scale):
    _need_cuda(q, k, v, dout, dq, dk, dv)
    check(load().vitmi_class_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), kv_stride, dout.data_ptr(),
                                      p_save.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dkv_stride,
                                      dtype_code(q), B, H, N, hd, float(scale), _stream()), "vitmi_class_attn_bwd")


def colsum_mul(x, y, out, *, M=None, N=None, ldx=None, ldy=None):
    _need_cuda(x, y, out)
    N = N or x.shape[-1]
    M = M or x.numel() // N
    lib = load()
    ws = workspace(lib.vitmi_colsum_mul_workspace(M, N), x.device)
    check(lib.vitmi_colsum_mul(x.data_ptr(), dtype_code(x), ldx or N, y.data_ptr(), dtype_code(y), ldy or N,
                               M, N, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "vitmi_colsum_mul")
    return out


def scale_cast(x, out, scale=None, *, M, N, ldx=None, ldo=None, rowscale=None, rows_per_group=0):
    """out[m, :N] = cast(x[m, :N] * scale * rowscale[m // rows_per_group]); rows at strides ldx / ldo."""
    _need_cuda(x, out)
    check(load().vitmi_scale_cast(x.data_ptr(), dtype_code(x), ldx or N, _ptr(scale), _ptr(rowscale),
                                  rows_per_group, out.data_ptr(), dtype_code(out), ldo or N, M, N, _stream()),
          "vitmi_scale_cast")
    return out


# ------------------------------------------------------------------ Swin ops ---
def win_attn_fwd(qkv, out, lse, bias, mask, Bw, H, N, hd, Himg, Wimg, ws, shift, scale):
    _need_cuda(qkv, out, lse, bias)
    check(load().vitmi_win_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), bias.data_ptr(), _ptr(mask),
                                    dtype_code(qkv), Bw, H, N, hd, Himg, Wimg, ws, shift, float(scale), _stream()),
          "vitmi_win_attn_fwd")


def win_attn_bwd_fuses_qkv_bias(t, hd) -> bool:
    return bool(load().vitmi_win_attn_bwd_fuses_qkv_bias(dtype_code(t), hd))


def win_attn_bwd(qkv, dout, lse, bias, mask, dqkv, dbias, Bw, H, N, hd, Himg, Wimg, ws, shift, scale,
                 dqkv_bias=None):
    """dqkv_bias: fp32 [3*H*hd] <- column sums of dqkv (only where win_attn_bwd_fuses_qkv_bias)."""
    _need_cuda(qkv, dout, dqkv, dbias)
    lib = load()
    ws_buf = workspace(lib.vitmi_win_attn_bwd_workspace(Bw, H, N), qkv.device)
    check(lib.vitmi_win_attn_bwd(qkv.data_ptr(), dout.data_ptr(), lse.data_ptr(), bias.data_ptr(), _ptr(mask),
                                 dqkv.data_ptr(), dbias.data_ptr(), _ptr(dqkv_bias), dtype_code(qkv), Bw, H, N, hd, Himg, Wimg, ws,
                                 shift, float(scale), ws_buf.data_ptr(), ws_buf.numel(), _stream()),
          "vitmi_win_attn_bwd")


def relpos_bias_gather(table, index, bias, T, H, N):
    check(load().vitmi_relpos_bias(table.data_ptr(), index.data_ptr(), bias.data_ptr(), None, None, T, H, N,
                                   _stream()), "vitmi_relpos_bias(gather)")


def relpos_bias_scatter(dbias, index, dtable, T, H, N):
    check(load().vitmi_relpos_bias(None, index.data_ptr(), None, dbias.data_ptr(), dtable.data_ptr(), T, H, N,
                                   _stream()), "vitmi_relpos_bias(scatter)")


def patch_merge(src, dst, B, Hh, Ww, Cc, inverse=False):
    _need_cuda(src, dst)
    assert src.dtype == dst.dtype
    check(load().vitmi_patch_merge(src.data_ptr(), dst.data_ptr(), dtype_code(src), B, Hh, Ww, Cc, int(inverse),
                                   _stream()), "vitmi_patch_merge")


def token_mean_fwd(x, out, B, L, Cc):
    check(load().vitmi_token_mean(x.data_ptr(), out.data_ptr(), None, None, dtype_code(x), B, L, Cc, _stream()),
          "vitmi_token_mean(fwd)")


def token_mean_bwd(dout, dx, B, L, Cc):
    check(load().vitmi_token_mean(None, None, dout.data_ptr(), dx.data_ptr(), dtype_code(dx), B, L, Cc, _stream()),
          "vitmi_token_mean(bwd)")
