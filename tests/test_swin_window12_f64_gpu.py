"""Window attention at windows of 65..144 tokens (windows 9..12) on the HIP path, against a float64 PyTorch reference
(tests/swin_util.py, itself pinned to the oracle's WindowAttention by test_swin_window12_ref_cpu.py): each of the four
template instances of the MFMA kernels with and without the shift mask, the vector kernels at every head dim, the
backward's walk of several windows per workgroup at the head counts of the 384-pixel models, determinism, the alignment
fallback, and the relative-position, PatchMerging and token-mean kernels at those models' shapes.

Error metric: max |got - want| / max |want| (util.rel_err).  Bounds: 2-3x the largest value measured on an MI355X over
all cases of the window sweep, the vector head dims and the walks (in brackets; every test prints its errors beside
their bounds with -s):
  * fp32-grade, FP32_GRADE = 2e-6.  Every output of the fp32 kernels [9.5e-7]; lse and d(bias) on both bf16 paths
    [lse 1.7e-7, dbias 4.9e-7]: in the MFMA kernels every score and dP entry is an fp32 sum of exact bf16 products,
    and d(bias) is an fp32 sum of fp32 dS over the windows of a walk and then over the workgroups.
  * bf16 vector kernels, VEC_OUT = VEC_DQKV = 7e-3: fp32 arithmetic and one rounding at the store, at most 2^-8 =
    3.9e-3 of the element [out 3.3e-3, dqkv 3.3e-3].
  * bf16 MFMA kernels, MFMA_OUT = 7e-3, MFMA_DQKV = 1.5e-2: O and dqkv also go through bf16-rounded P (forward) and
    P / dS (backward), a second error of the same order, spread over the 81..144-term contraction [out 3.2e-3, dqkv
    6.0e-3].
  * The MFMA backward's fused qkv-bias sums, QKV_BIAS = 1.5e-3: fp32 sums of the fp32 dQ / dK / dV accumulators, whose
    bf16-rounded P / dS operands leave errors that largely cancel over a column [5.3e-4].
"""
import functools

import pytest
import torch

from swin_util import (F64, WALKS12, bits, check, compare as _compare, dev_err, drop_margins, gen, inputs, nan, run,
                       torch_window_attention, walk_shape)

pytestmark = pytest.mark.gpu

FP32_GRADE = 2e-6                      # lse / dbias everywhere; every output of the fp32 kernels
VEC_OUT, VEC_DQKV = 7e-3, 7e-3         # bf16 vector kernels
MFMA_OUT, MFMA_DQKV = 7e-3, 1.5e-2     # bf16 MFMA kernels
QKV_BIAS = 1.5e-3                      # fused qkv-bias sums of the MFMA backward
W12 = dict(FP32_GRADE=FP32_GRADE, VEC_OUT=VEC_OUT, VEC_DQKV=VEC_DQKV, MFMA_OUT=MFMA_OUT, MFMA_DQKV=MFMA_DQKV,
           QKV_BIAS=QKV_BIAS)


@pytest.fixture(scope="module")
def ops(lib):
    from vit_torch_amd import ops as _o
    return _o


@functools.lru_cache(maxsize=2)
def reference(B, Hh, Ww, ws, shift, H, hd, seed, images_per_chunk=None):
    """(qkv, do, bias, float64 reference) of a shape: computed once for the paths of a case, which run back to back."""
    qkv, do, bias = inputs(B, Hh, Ww, ws, H, hd, seed)
    return qkv, do, bias, torch_window_attention(qkv, do, bias, B, Hh, Ww, ws, shift, H, hd, F64, images_per_chunk)


def compare(ops, lib, path, B, Hh, Ww, ws, shift, H, hd, seed, tag, images_per_chunk=None, force=True):
    return _compare(W12, ops, lib, path, B, Hh, Ww, ws, shift, H, hd, seed, tag, force=force,
                    ref=reference(B, Hh, Ww, ws, shift, H, hd, seed, images_per_chunk))


# ------------------------------------------------------------------------------------------- a. window sweep ---
# two images of 2 x 3 windows (non-square, so rows and columns cannot be confused).  N = 81 has one live row in query
# block 5, N = 121 a scalar d(bias) tail, N = 100 ends on a vector boundary
SWEEP = [(ws, shift, 2, 32) for ws in (9, 10, 11, 12) for shift in (0, ws // 2)]
# hd 64 at ws 12 is the largest LDS request of the vector kernels (4 * 144 * 65 floats)
SWEEP_VEC = [(12, 6, 2, 64), (12, 0, 3, 48), (12, 6, 2, 24), (12, 0, 2, 8), (11, 5, 2, 64), (11, 0, 3, 16), (11, 5, 3, 8),
             (10, 5, 2, 48), (10, 0, 2, 24), (10, 5, 3, 16), (9, 4, 3, 64), (9, 0, 2, 48), (9, 4, 2, 8)]


@pytest.mark.parametrize("path", ["fp32", "vector", "mfma"])
@pytest.mark.parametrize("ws,shift,H,hd", SWEEP)
def test_window_sweep_hd32(ops, lib, path, ws, shift, H, hd):
    compare(ops, lib, path, 2, 2 * ws, 3 * ws, ws, shift, H, hd, 100 + ws, f"ws{ws}s{shift}.{path}")


@pytest.mark.parametrize("path", ["fp32", "vector"])
@pytest.mark.parametrize("ws,shift,H,hd", SWEEP_VEC)
def test_window_sweep_vector_head_dims(ops, lib, path, ws, shift, H, hd):
    """hd != 32 takes the fp32 vector kernels in both dtypes with the MFMA switch at its default."""
    compare(ops, lib, path, 2, 2 * ws, 3 * ws, ws, shift, H, hd, 200 + hd, f"ws{ws}s{shift}hd{hd}.{path}", force=False)


# ------------------------------------------------------------------------------------ c. walks, against fp64 ---
@pytest.mark.parametrize("path", ["mfma", "vector", "fp32"])
@pytest.mark.parametrize("case", list(WALKS12))
def test_walk_against_float64(ops, lib, path, case):
    """A backward workgroup walks windows r, r + R, ..., accumulating d(bias) in place in its partial row behind a
    `first` flag (the MFMA kernel and the vector dQ kernel alike), the qkv-bias sums in LDS, and taking the mask window
    bw % nW anew at every step.  Dropping one window of a walk would take that (window, head)'s d(score) tile out of
    dbias and its dq/dk/dv column sums out of dqkv_bias; the reference measures both for every (window, head).  The
    smallest over all cases: dbias 5.2e-2 (h3), 25000x FP32_GRADE; qkv-bias sums 3.5e-2 (h3), 23x QKV_BIAS.  The test
    requires at least 4x for both."""
    B, Hh, Ww, ws, shift, H, Bw, R = walk_shape(case)
    hd = 32
    r, eb, eq = compare(ops, lib, path, B, Hh, Ww, ws, shift, H, hd, 300 + H + ws, f"walk.{case}.{path}",
                        images_per_chunk=8)
    drop_b, drop_q = drop_margins(r, H, hd)
    print(f"\n  walk.{case}: Bw {Bw}, R {R}, {Bw // R}-{-(-Bw // R)} windows per workgroup; one dropped window moves "
          f"dbias by >= {drop_b:.2e} (bound {FP32_GRADE:.1e}), dqkv_bias by >= {drop_q:.2e} (bound {QKV_BIAS:.1e})", end="")
    assert FP32_GRADE * 4 <= drop_b
    assert QKV_BIAS * 4 <= drop_q


# ------------------------------------------------------------------------- d. MFMA against vector, same bits ---
@pytest.mark.parametrize("case", ["h24", "h48_long"])
def test_walk_mfma_against_vector(ops, lib, case):
    """The MFMA kernels against the fp32 vector kernels on the same bf16 inputs, compared on the device.  Bounds: the
    two paths' bounds against float64 added; the fused qkv-bias sums against float64 column sums of the vector path's
    dqkv."""
    B, Hh, Ww, ws, shift, H, Bw, R = walk_shape(case)
    hd = 32
    qkv, do, bias = inputs(B, Hh, Ww, ws, H, hd, 300 + H + ws)
    from oracle.swin_ref import shift_attn_mask
    mask = shift_attn_mask(Hh, Ww, ws, shift) if shift else None
    assert ops.win_attn_bwd_fuses_qkv_bias(torch.empty(1, dtype=torch.bfloat16), hd)
    Om, lm, dqm, dbm, qbm = run(ops, qkv, do, bias, mask, B, Hh, Ww, ws, shift, H, hd, torch.bfloat16, qkv_bias=True)
    lib.vitmi_debug_win_attn_mfma(0)
    Ov, lv, dqv, dbv, _ = run(ops, qkv, do, bias, mask, B, Hh, Ww, ws, shift, H, hd, torch.bfloat16)
    errs = {"out": (dev_err(Om, Ov), MFMA_OUT + VEC_OUT), "lse": (dev_err(lm, lv), 2 * FP32_GRADE),
            "dqkv": (dev_err(dqm, dqv), MFMA_DQKV + VEC_DQKV), "dbias": (dev_err(dbm, dbv), 2 * FP32_GRADE),
            "dqkv_bias": (dev_err(qbm, dqv.view(-1, 3 * H * hd).double().sum(0)), QKV_BIAS)}
    for k, (e, b) in errs.items():
        print(f"\n  walk.{case} mfma vs vector {k}: {e:.2e} (bound {b:.1e})", end="")
    for k, (e, b) in errs.items():
        assert e <= b, f"{k}: {e:.3e} > {b:.1e}"


# ------------------------------------------------------------------------------------------- e. determinism ---
@pytest.mark.parametrize("path", ["mfma", "vector"])
def test_walk_is_deterministic(ops, lib, path):
    """Forward and backward twice at h24 (2-3 windows per workgroup, the mask window alternating): the same bits."""
    if path == "vector":
        lib.vitmi_debug_win_attn_mfma(0)
    B, Hh, Ww, ws, shift, H, Bw, R = walk_shape("h24")
    hd = 32
    qkv, do, bias = inputs(B, Hh, Ww, ws, H, hd, 400)
    from oracle.swin_ref import shift_attn_mask
    mask = shift_attn_mask(Hh, Ww, ws, shift)
    fuse = path == "mfma"
    a = run(ops, qkv, do, bias, mask, B, Hh, Ww, ws, shift, H, hd, torch.bfloat16, qkv_bias=fuse)
    b = run(ops, qkv, do, bias, mask, B, Hh, Ww, ws, shift, H, hd, torch.bfloat16, qkv_bias=fuse)
    assert (a[4] is not None) == fuse
    for x, y in zip(a, b):
        if x is not None:
            assert not x.isnan().any() and torch.equal(bits(x), bits(y))


# ---------------------------------------------------------------------------------------------- f. alignment ---
def test_unaligned_views_fall_back_to_the_vector_kernels(ops, lib):
    """bf16 qkv / out / dqkv views one element (2 bytes) off: the MFMA kernels need 16- / 8-byte rows, so the dispatch
    takes the vector kernels at N > 64 too.  Their results match float64 at the vector bounds and equal, bit for bit,
    the vector kernels on aligned copies.  Asking for the fused qkv-bias sums on such views is refused before anything
    runs."""
    from vit_torch_amd._lib import VitmiError
    B, Hh, Ww, ws, shift, H, hd = 2, 24, 36, 12, 6, 3, 32
    C, N, L = H * hd, ws * ws, Hh * Ww
    Bw = B * (Hh // ws) * (Ww // ws)
    scale = hd ** -0.5
    qkv, do, bias = inputs(B, Hh, Ww, ws, H, hd, 500)
    r = torch_window_attention(qkv, do, bias, B, Hh, Ww, ws, shift, H, hd, F64)
    md, bd = r.mask.cuda().contiguous(), bias.cuda().contiguous()
    dO = do.to("cuda", torch.bfloat16).contiguous()

    def off(shape):
        n = 1
        for s in shape:
            n *= s
        t = torch.full((n + 1,), float("nan"), device="cuda", dtype=torch.bfloat16)[1:].view(shape)
        assert t.data_ptr() % 16 == 2
        return t

    Q = off((B, L, 3 * C))
    Q.copy_(qkv.to(torch.bfloat16))
    O, lse = off((B, L, C)), nan((Bw * H * N,), torch.float32)
    ops.win_attn_fwd(Q, O, lse, bd, md, Bw, H, N, hd, Hh, Ww, ws, shift, scale)
    dqkv, dbias = off((B, L, 3 * C)), nan((H * N * N,), torch.float32)
    ops.win_attn_bwd(Q, dO, lse, bd, md, dqkv, dbias, Bw, H, N, hd, Hh, Ww, ws, shift, scale)
    check("unaligned.out", O, r.out, VEC_OUT)
    check("unaligned.lse", lse, r.lse, FP32_GRADE)
    check("unaligned.dqkv", dqkv, r.dqkv, VEC_DQKV)
    check("unaligned.dbias", dbias.view(H, N, N), r.dbias, FP32_GRADE)
    lib.vitmi_debug_win_attn_mfma(0)
    O2, lse2, dqkv2, dbias2, _ = run(ops, qkv, do, bias, r.mask, B, Hh, Ww, ws, shift, H, hd, torch.bfloat16)
    lib.vitmi_debug_win_attn_mfma(-1)
    assert torch.equal(bits(O), bits(O2)) and torch.equal(bits(lse), bits(lse2))
    assert torch.equal(bits(dqkv), bits(dqkv2)) and torch.equal(bits(dbias.view(H, N, N)), bits(dbias2))
    # the fused qkv-bias sums exist on the MFMA kernel only: refused on these views, with nothing written
    assert ops.win_attn_bwd_fuses_qkv_bias(Q, hd)
    dqkv3, dbias3, qb = off((B, L, 3 * C)), nan((H * N * N,), torch.float32), nan((3 * C,), torch.float32)
    with pytest.raises(VitmiError, match="dqkv_bias"):
        ops.win_attn_bwd(Q, dO, lse, bd, md, dqkv3, dbias3, Bw, H, N, hd, Hh, Ww, ws, shift, scale, dqkv_bias=qb)
    torch.cuda.synchronize()
    assert dqkv3.isnan().all() and dbias3.isnan().all() and qb.isnan().all()


# -------------------------------------------------------------------------------- g. relative-position bias ---
@pytest.mark.parametrize("H", [4, 6, 32, 48])
@pytest.mark.parametrize("ws", [9, 10, 11, 12])
def test_relpos_bias_gather_scatter(ops, ws, H):
    """Gather: exactly the indexed table.  Scatter (deterministic per-row compaction into an LDS list of 256 slots):
    within 1e-6 of a float64 index_add_, and the same bits on a repeat.  The centre table row (relative position (0, 0))
    has N matches, the diagonal: the fullest list of any row, checked on its own."""
    from oracle.swin_ref import relative_position_index
    N, T = ws * ws, (2 * ws - 1) ** 2
    table = gen((T, H), ws)
    idx = relative_position_index(ws)
    want = table[idx.view(-1)].view(N, N, H).permute(2, 0, 1)
    bias = torch.full((H * N * N,), float("nan"), device="cuda")
    ops.relpos_bias_gather(table.cuda(), idx.cuda(), bias, T, H, N)
    assert torch.equal(bias.view(H, N, N).cpu(), want)
    db = gen((H, N, N), 10 + ws)
    want_dt = torch.zeros(T, H, dtype=F64).index_add_(0, idx.view(-1), db.to(F64).permute(1, 2, 0).reshape(N * N, H))
    dt = torch.full((T, H), float("nan"), device="cuda")
    ops.relpos_bias_scatter(db.cuda().contiguous(), idx.cuda(), dt, T, H, N)
    check(f"relpos.ws{ws}.H{H}.dtable", dt, want_dt, 1e-6)
    centre = T // 2
    assert (idx == centre).sum().item() == N and torch.bincount(idx.view(-1), minlength=T).max().item() == N
    check(f"relpos.ws{ws}.H{H}.dtable[centre]", dt[centre], db.to(F64).diagonal(dim1=1, dim2=2).sum(1), 1e-6)
    dt2 = torch.full((T, H), float("nan"), device="cuda")
    ops.relpos_bias_scatter(db.cuda().contiguous(), idx.cuda(), dt2, T, H, N)
    assert torch.equal(bits(dt), bits(dt2))


# ------------------------------------------------------------------------------ h. patch merge, token mean ---
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Hh,C", [(96, 128), (48, 256), (24, 512), (24, 768)])
def test_patch_merge_at_swin_384_stage_shapes(ops, dt, Hh, C):
    """PatchMerging's gather and its inverse after stages 1-3 of swin_base (C 128..512) and at swin_large's stage 3
    (C 768) at 384 pixels: a permutation, so exact."""
    B = 2
    x = gen((B, Hh * Hh, C), Hh).to(dt)
    xv = x.view(B, Hh, Hh, C)
    want = torch.cat([xv[:, 0::2, 0::2], xv[:, 1::2, 0::2], xv[:, 0::2, 1::2], xv[:, 1::2, 1::2]], -1)
    out = torch.full((B, Hh * Hh // 4, 4 * C), float("nan"), device="cuda", dtype=dt)
    ops.patch_merge(x.cuda(), out, B, Hh, Hh, C)
    assert torch.equal(out.cpu(), want.reshape(B, -1, 4 * C))
    back = torch.full((B, Hh * Hh, C), float("nan"), device="cuda", dtype=dt)
    ops.patch_merge(out, back, B, Hh, Hh, C, inverse=True)
    assert torch.equal(back.cpu(), x)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1024, 1536])
def test_token_mean_at_swin_384_head_shapes(ops, dt, C):
    """The mean over the 144 final tokens of swin_base / swin_large at 384 pixels against float64 (an fp32 sum of 144
    terms); the backward is one fp32 division and one rounding, so it equals dout / L rounded to the dtype exactly."""
    B, L = 2, 144
    x = gen((B, L, C), 7).to(dt)
    m = torch.full((B, C), float("nan"), device="cuda")
    ops.token_mean_fwd(x.cuda(), m, B, L, C)
    check(f"token_mean.C{C}.{dt}", m, x.to(F64).mean(1), 1e-6)
    dm = gen((B, C), 8)
    dx = torch.full((B, L, C), float("nan"), device="cuda", dtype=dt)
    ops.token_mean_bwd(dm.cuda(), dx, B, L, C)
    assert torch.equal(dx.cpu(), (dm / L).to(dt).unsqueeze(1).expand(B, L, C))
