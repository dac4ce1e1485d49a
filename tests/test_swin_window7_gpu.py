"""Window attention at windows of N <= 64 tokens (window 7 and its neighbours 4..8) on the HIP path, against a float64
PyTorch reference (tests/swin_util.py), at the shapes where the kernels go wrong: every window size and head dim the
dispatch can take, the bf16 MFMA backward's walk of several windows per wave at reduced size and at Swin-T batch-256
stage shapes, determinism, the alignment fallback, and the relative-position, PatchMerging and token-mean kernels.

Error metric: max |got - want| / max |want| (util.rel_err).  Bounds, from the kernels' arithmetic, each about 2-3x
the largest value measured on an MI355X (in brackets; every test prints its errors beside their bounds with -s):
  * fp32-grade, FP32_GRADE = 2e-6.  The fp32 kernels compute and store in fp32 [7e-7].  lse and d(bias) on both bf16
    paths are fp32-grade too: in the MFMA kernels every score and dP entry is an fp32 sum of exact bf16 products, and
    d(bias) is an fp32 sum of fp32 dS over windows [lse 2e-7, dbias 5e-7].
  * bf16 vector kernels, VEC = 6e-3: fp32 arithmetic and one rounding at the store, at most 2^-8 = 3.9e-3 of the
    element [out 3.4e-3, dqkv 3.0e-3].
  * bf16 MFMA kernels: O and dqkv also go through bf16-rounded P (forward) and P / dS (backward), a second error of
    the same order, spread over the N-term contraction [out 3.3e-3, dqkv 4.4e-3].
  * The MFMA backward's fused qkv-bias sums are fp32 sums of the fp32 dQ / dK / dV accumulators, whose bf16-rounded
    P / dS operands leave errors that largely cancel over a column [8.4e-4].
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from swin_util import check, compare as _compare, dev_err, gen, inputs, nan, run, torch_window_attention, window_tokens
from util import cosine, rel_err

pytestmark = pytest.mark.gpu

F64 = torch.float64
FP32_GRADE = 2e-6                      # lse / dbias everywhere; every output of the fp32 kernels
VEC_OUT, VEC_DQKV = 6e-3, 6e-3         # bf16 vector kernels
MFMA_OUT, MFMA_DQKV = 8e-3, 1e-2       # bf16 MFMA kernels
QKV_BIAS = 1.5e-3                      # fused qkv-bias sums of the MFMA backward


W7 = dict(FP32_GRADE=FP32_GRADE, VEC_OUT=VEC_OUT, VEC_DQKV=VEC_DQKV, MFMA_OUT=MFMA_OUT, MFMA_DQKV=MFMA_DQKV,
          QKV_BIAS=QKV_BIAS)
compare = functools.partial(_compare, W7)


@pytest.fixture(scope="module")
def ops(lib):
    from vit_torch_amd import ops as _o
    return _o


# ------------------------------------------------------------------------------------------- 1. window sweep ---
# images of 2 x 3 windows (non-square, so rows and columns cannot be confused), two of them
SWEEP = [(ws, shift, 2, 32) for ws in (4, 5, 6, 7, 8) for shift in (0, ws // 2)]
SWEEP_VEC = [(8, 4, 2, 24), (8, 0, 2, 64), (8, 4, 3, 48), (7, 3, 2, 24), (7, 0, 2, 64), (7, 3, 3, 48), (6, 3, 2, 16),
             (6, 0, 3, 8), (5, 2, 2, 64), (5, 0, 2, 24), (4, 2, 3, 48), (4, 0, 2, 16), (8, 4, 4, 8)]


@pytest.mark.parametrize("path", ["fp32", "vector", "mfma"])
@pytest.mark.parametrize("ws,shift,H,hd", SWEEP)
def test_window_sweep_hd32(ops, lib, path, ws, shift, H, hd):
    compare(ops, lib, path, 2, 2 * ws, 3 * ws, ws, shift, H, hd, 100 + ws, f"ws{ws}s{shift}.{path}")


@pytest.mark.parametrize("path", ["fp32", "vector"])
@pytest.mark.parametrize("ws,shift,H,hd", SWEEP_VEC)
def test_window_sweep_vector_head_dims(ops, lib, path, ws, shift, H, hd):
    """hd != 32 takes the fp32 vector kernels in both dtypes with the MFMA switch at its default."""
    compare(ops, lib, path, 2, 2 * ws, 3 * ws, ws, shift, H, hd, 200 + hd, f"ws{ws}s{shift}hd{hd}.{path}", force=False)


# ------------------------------------------------------------------------------------ 2. walks, against fp64 ---
def per_head(H, Bw):
    """windows a backward wave walks are wid/H, wid/H + per_head, ... (swin_ops.hip, the N <= 64 MFMA dispatch)."""
    return max(1, min(1024 // H, Bw))


# (B, Hh, Ww, shift, H): Bw = B * nW windows of 49 tokens, per_head = min(1024 // H, Bw)
WALKS = {
    # H = 3: per_head 341, 1023 waves (the last workgroup runs 3 of its 4), Bw 1416 = 4 * 341 + 52: 4 or 5 windows
    # per wave; shift 3 with 4 windows per image, and 341 % 4 = 1: the mask window changes at every step of a walk
    "h3": (354, 14, 14, 3, 3),
    # H = 24 as in Swin-B/L stage 4 (7 x 7, one window, no shift): per_head 42, Bw 100 = 2 * 42 + 16: 2 or 3 windows
    "h24": (100, 7, 7, 0, 24),
    # H = 6, 28 x 28 (16 windows per image), shift 3: per_head 170, Bw 384 = 2 * 170 + 44, 170 % 16 = 10
    "h6": (24, 28, 28, 3, 6),
}


@pytest.mark.parametrize("path", ["mfma", "vector"])
@pytest.mark.parametrize("case", list(WALKS))
def test_walk_against_float64(ops, lib, path, case):
    """The MFMA backward's waves walk several windows, accumulating d(bias), the qkv-bias sums and the mask phase
    across the walk (the vector kernels, one workgroup per window, on the same inputs).  Dropping one window of a
    walk would take that (window, head)'s d(score) tile out of dbias and its dq/dk/dv column sums out of dqkv_bias.
    The reference measures that effect for every (window, head) as max |tile| / max |dbias|, and likewise for the
    column sums.  With random inputs the sums over windows grow like sqrt(Bw), so the effect is about one part in
    sqrt(Bw), not in Bw: the smallest measured is 1.5e-2 for dbias, 7700x FP32_GRADE, and 9.0e-3 for the qkv-bias
    sums, 6x QKV_BIAS (at h3, the longest walk).  The test requires at least 4x for both."""
    B, Hh, Ww, shift, H = WALKS[case]
    ws, hd = 7, 32
    Bw = B * (Hh // ws) * (Ww // ws)
    ph = per_head(H, Bw)
    assert Bw > ph and Bw % ph != 0
    r, eb, eq = compare(ops, lib, path, B, Hh, Ww, ws, shift, H, hd, 300 + H, f"walk.{case}.{path}", images_per_chunk=16)
    drop_b = (r.ds_max / r.dbias.abs().max()).min().item()
    print(f"\n  walk.{case}: Bw {Bw}, per_head {ph}, {Bw // ph}-{-(-Bw // ph)} windows per wave; "
          f"one dropped window moves dbias by >= {drop_b:.2e} (bound {FP32_GRADE:.1e})", end="")
    assert FP32_GRADE * 4 <= drop_b
    if eq is not None:
        qref = r.dqkv.reshape(-1, 3 * H * hd).sum(0)
        drop_q = (r.qb_max / qref.abs().max()).min().item()
        print(f"; dqkv_bias by >= {drop_q:.2e} (bound {QKV_BIAS:.1e})", end="")
        assert QKV_BIAS * 4 <= drop_q


# ---------------------------------------------------------------------- 3. walks at Swin-T batch-256 stages ---
# Swin-T (benchmark config C5, batch 256): (H, resolution, shift); stage 4 is one 7 x 7 window, so unshifted
C5_STAGES = [(3, 56, 3), (6, 28, 3), (12, 14, 3), (24, 7, 0)]


@pytest.mark.parametrize("stage", [1, 2, 3, 4])
def test_walk_at_swin_t_batch256_stage_shapes(ops, lib, stage):
    """The MFMA kernels against the fp32 vector kernels on the same random bf16 inputs, at Swin-T's four stage shapes
    at batch 256: 48-49 / 24-25 / 12-13 / 6-7 windows per backward wave.  Bounds: the two paths' bounds against
    float64 added.  The MFMA backward with its L2 prefetch of the next window switched off gives the same bits.  The
    fused qkv-bias sums against float64 column sums of the vector path's dqkv.  The effect of dropping one window is
    measured by a vector backward whose dO is zero outside that window (its dbias is then that window's tile), for four
    sampled windows.  Measured smallest effects, stages 1-4: dbias 1.1e-2 / 1.6e-2 / 2.5e-2 / 5.0e-2, at least 2700x
    its bound 2 * FP32_GRADE; qkv-bias sums 3.9e-3 / 1.1e-2 / 1.6e-2 / 3.2e-2, at least 2.6x QKV_BIAS.  The test
    requires 4x and 2x: over 16384 windows a single one moves a column sum only by about 1 / sqrt(16384)."""
    H, R, shift = C5_STAGES[stage - 1]
    B, ws, hd = 256, 7, 32
    C, N, L, nW = H * hd, ws * ws, R * R, (R // ws) ** 2
    Bw = B * nW
    scale = hd ** -0.5
    g = torch.Generator(device="cuda").manual_seed(stage)
    Q = torch.randn((B, L, 3 * C), device="cuda", generator=g).to(torch.bfloat16)
    dO = torch.randn((B, L, C), device="cuda", generator=g).to(torch.bfloat16)
    bias = (torch.randn((H, N, N), device="cuda", generator=g) * 0.5).contiguous()
    from oracle.swin_ref import shift_attn_mask
    md = shift_attn_mask(R, R, ws, shift).cuda().contiguous() if shift else None

    def fwd():
        O, lse = nan((B, L, C), torch.bfloat16), nan((Bw * H * N,), torch.float32)
        ops.win_attn_fwd(Q, O, lse, bias, md, Bw, H, N, hd, R, R, ws, shift, scale)
        return O, lse

    def bwd(lse, dout, qkv_bias):
        dqkv, dbias = nan((B, L, 3 * C), torch.bfloat16), nan((H * N * N,), torch.float32)
        qb = nan((3 * C,), torch.float32) if qkv_bias else None
        ops.win_attn_bwd(Q, dout, lse, bias, md, dqkv, dbias, Bw, H, N, hd, R, R, ws, shift, scale, dqkv_bias=qb)
        return dqkv, dbias.view(H, N, N), qb

    ph = per_head(H, Bw)
    assert ops.win_attn_bwd_fuses_qkv_bias(Q, hd)
    Om, lm = fwd()
    dqm, dbm, qbm = bwd(lm, dO, True)
    lib.vitmi_debug_win_bwd_prefetch(0)
    dqp, dbp, qbp = bwd(lm, dO, True)
    lib.vitmi_debug_win_bwd_prefetch(1)
    assert torch.equal(dqp.view(torch.int16), dqm.view(torch.int16))
    assert torch.equal(dbp, dbm) and torch.equal(qbp, qbm)
    lib.vitmi_debug_win_attn_mfma(0)
    Ov, lv = fwd()
    dqv, dbv, _ = bwd(lv, dO, False)
    errs = {"out": (dev_err(Om, Ov), MFMA_OUT + VEC_OUT), "lse": (dev_err(lm, lv), 2 * FP32_GRADE),
            "dqkv": (dev_err(dqm, dqv), MFMA_DQKV + VEC_DQKV), "dbias": (dev_err(dbm, dbv), 2 * FP32_GRADE)}
    qref = dqv.view(-1, 3 * C).double().sum(0)
    errs["dqkv_bias"] = (dev_err(qbm, qref), QKV_BIAS)
    # one window's d(score) tile and dq/dk/dv column sums, per head, at four sampled windows
    drop_b, drop_q = float("inf"), float("inf")
    for bw in (0, nW - 1, Bw // 2 + 1, Bw - 1):
        mask_rows = torch.zeros(B * L, device="cuda", dtype=torch.bool)
        mask_rows[window_tokens(R, R, ws, shift, bw, nW).cuda()] = True
        dO1 = torch.where(mask_rows.view(B, L, 1), dO, torch.zeros_like(dO))
        dq1, db1, _ = bwd(lv, dO1, False)
        drop_b = min(drop_b, (db1.abs().amax((1, 2)) / dbv.abs().max()).min().item())
        cs = dq1.view(-1, 3, H, hd).double().sum(0).abs().amax((0, 2))
        drop_q = min(drop_q, (cs / qref.abs().max()).min().item())
    print(f"\n  C5 stage {stage}: H {H}, Bw {Bw}, per_head {ph}, {Bw // ph}-{-(-Bw // ph)} windows per wave", end="")
    for k, (e, b) in errs.items():
        print(f"\n  C5 stage {stage} mfma vs vector {k}: {e:.2e} (bound {b:.1e})", end="")
    print(f"\n  C5 stage {stage}: one dropped window moves dbias by >= {drop_b:.2e}, dqkv_bias by >= {drop_q:.2e}", end="")
    for k, (e, b) in errs.items():
        assert e <= b, f"{k}: {e:.3e} > {b:.1e}"
    assert 4 * 2 * FP32_GRADE <= drop_b and 2 * QKV_BIAS <= drop_q


# ------------------------------------------------------------------------------------------- 4. determinism ---
@pytest.mark.parametrize("path", ["mfma", "vector"])
def test_walk_is_deterministic(ops, lib, path):
    """Forward and backward twice at a walk shape (H = 6, 28 x 28, shift 3, Bw 512: 3-4 windows per wave): the same
    bits."""
    if path == "vector":
        lib.vitmi_debug_win_attn_mfma(0)
    B, Hh, Ww, ws, shift, H, hd = 32, 28, 28, 7, 3, 6, 32
    qkv, do, bias = inputs(B, Hh, Ww, ws, H, hd, 400)
    from oracle.swin_ref import shift_attn_mask
    mask = shift_attn_mask(Hh, Ww, ws, shift)
    fuse = path == "mfma"
    a = run(ops, qkv, do, bias, mask, B, Hh, Ww, ws, shift, H, hd, torch.bfloat16, qkv_bias=fuse)
    b = run(ops, qkv, do, bias, mask, B, Hh, Ww, ws, shift, H, hd, torch.bfloat16, qkv_bias=fuse)
    for x, y in zip(a, b):
        if x is not None:
            assert torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32),
                               y.view(torch.int16) if y.dtype == torch.bfloat16 else y.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 5. alignment ---
def test_unaligned_views_fall_back_to_the_vector_kernels(ops, lib):
    """bf16 qkv / out / dqkv views one element (2 bytes) off: the MFMA kernels need 16- / 8-byte rows, so the dispatch
    takes the vector kernels.  Their results match float64 at the vector bounds and equal, bit for bit, the vector
    kernels on aligned copies.  Asking for the fused qkv-bias sums on such views is refused before anything runs."""
    from vit_torch_amd._lib import VitmiError
    B, Hh, Ww, ws, shift, H, hd = 2, 14, 21, 7, 3, 3, 32
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
    assert torch.equal(O.view(torch.int16), O2.view(torch.int16)) and torch.equal(lse, lse2)
    assert torch.equal(dqkv.view(torch.int16), dqkv2.view(torch.int16)) and torch.equal(dbias.view(H, N, N), dbias2)
    # the fused qkv-bias sums exist on the MFMA kernel only: refused on these views, with nothing written
    assert ops.win_attn_bwd_fuses_qkv_bias(Q, hd)
    dqkv3, dbias3, qb = off((B, L, 3 * C)), nan((H * N * N,), torch.float32), nan((3 * C,), torch.float32)
    with pytest.raises(VitmiError, match="dqkv_bias"):
        ops.win_attn_bwd(Q, dO, lse, bd, md, dqkv3, dbias3, Bw, H, N, hd, Hh, Ww, ws, shift, scale, dqkv_bias=qb)
    torch.cuda.synchronize()
    assert dqkv3.isnan().all() and dbias3.isnan().all() and qb.isnan().all()


# -------------------------------------------------------------------------------- 6. relative-position bias ---
@pytest.mark.parametrize("ws,H", [(2, 48), (3, 1), (4, 24), (5, 3), (6, 32), (7, 48), (8, 24), (8, 48)])
def test_relpos_bias_gather_scatter(ops, ws, H):
    """Gather: exactly the indexed table.  Scatter (deterministic per-row compaction; at ws 8 its LDS list of
    64 * 64 slots is full): within 1e-6 of a float64 index_add_, and the same bits on a repeat."""
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
    dt2 = torch.full((T, H), float("nan"), device="cuda")
    ops.relpos_bias_scatter(db.cuda().contiguous(), idx.cuda(), dt2, T, H, N)
    assert torch.equal(dt, dt2)


# ------------------------------------------------------------------------------ 7. patch merge, token mean ---
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Hh,C", [(56, 96), (28, 192), (14, 384)])
def test_patch_merge_at_swin_t_stage_shapes(ops, dt, Hh, C):
    B = 8
    x = gen((B, Hh * Hh, C), Hh).to(dt)
    xv = x.view(B, Hh, Hh, C)
    want = torch.cat([xv[:, 0::2, 0::2], xv[:, 1::2, 0::2], xv[:, 0::2, 1::2], xv[:, 1::2, 1::2]], -1)
    out = torch.full((B, Hh * Hh // 4, 4 * C), float("nan"), device="cuda", dtype=dt)
    ops.patch_merge(x.cuda(), out, B, Hh, Hh, C)
    assert torch.equal(out.cpu(), want.reshape(B, -1, 4 * C))
    back = torch.full((B, Hh * Hh, C), float("nan"), device="cuda", dtype=dt)
    ops.patch_merge(out, back, B, Hh, Hh, C, inverse=True)
    assert torch.equal(back.cpu(), x)


@pytest.mark.parametrize("Hh,Ww,C", [(7, 8, 16), (8, 7, 16), (8, 8, 6)])
def test_patch_merge_refuses_odd_sides_and_channels(ops, Hh, Ww, C):
    from vit_torch_amd._lib import VitmiError
    x = torch.zeros((1, Hh * Ww, C), device="cuda")
    out = torch.zeros((1, Hh * Ww, C), device="cuda")
    with pytest.raises(VitmiError, match="even"):
        ops.patch_merge(x, out, 1, Hh, Ww, C)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_token_mean_at_swin_t_head_shape(ops, dt):
    """The mean over Swin-T's 49 final tokens of 768 channels against float64 (an fp32 sum of 49 terms); the backward
    is one fp32 division and one rounding, so it equals dout / L rounded to the dtype exactly."""
    B, L, C = 8, 49, 768
    x = gen((B, L, C), 7).to(dt)
    m = torch.full((B, C), float("nan"), device="cuda")
    ops.token_mean_fwd(x.cuda(), m, B, L, C)
    check(f"token_mean.{dt}", m, x.to(F64).mean(1), 1e-6)
    dm = gen((B, C), 8)
    dx = torch.full((B, L, C), float("nan"), device="cuda", dtype=dt)
    ops.token_mean_bwd(dm.cuda(), dx, B, L, C)
    assert torch.equal(dx.cpu(), (dm / L).to(dt).unsqueeze(1).expand(B, L, C))


# ------------------------------------------------------------------------------ 8. models against the oracle ---
# (cfg, batch, image size): a hd 32 window-7 model whose stage 1 walks (56 x 56 tokens, 2 heads: Bw = 64 B = 704 >
# per_head 512 at B = 11), and two window-8 models (64 x 64, patch 4: 16 x 16 tokens, 4 windows, then one 8 x 8
# window) at hd 32 and at hd 24 (swin_tiny_c24_patch4_window8_256's head dim)
MODELS = {
    "w7_hd32_walk": (dict(img_size=224, patch_size=4, in_chans=3, num_classes=10, embed_dim=64, depths=[2, 2],
                          num_heads=[2, 4], window_size=7, drop_path_rate=0.0), 11),
    "w8_hd32": (dict(img_size=64, patch_size=4, in_chans=3, num_classes=10, embed_dim=64, depths=[2, 2],
                     num_heads=[2, 4], window_size=8, drop_path_rate=0.0), 4),
    "w8_hd24": (dict(img_size=64, patch_size=4, in_chans=3, num_classes=10, embed_dim=48, depths=[2, 2],
                     num_heads=[2, 4], window_size=8, drop_path_rate=0.0), 4),
}


def make_pair(cfg, compute, residual="fp32"):
    from oracle.swin_ref import SwinTransformer as Ref
    from oracle.vit_ref import seeded_init_
    from vit_torch_amd import SwinTransformer
    ref = Ref(**cfg)
    seeded_init_(ref, 7)
    m = SwinTransformer(**cfg, compute_dtype=compute, residual_dtype=residual)
    res = m.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return ref, m.cuda()


def step(ref, m, B, S):
    from vit_torch_amd import CrossEntropyLoss
    g = torch.Generator("cpu").manual_seed(0)
    x, y = torch.randn(B, 3, S, S, generator=g), torch.randint(0, 10, (B,), generator=g)
    lo = ref(x)
    lr = F.cross_entropy(lo, y)
    ref.zero_grad(); lr.backward()
    out = m(x.cuda())
    loss = CrossEntropyLoss()(out, y.cuda())
    m.zero_grad(); loss.backward()
    return lo.detach(), lr.detach(), out.detach(), loss.detach()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("model", list(MODELS))
def test_tiny_swin_against_oracle(model, compute):
    """Per-parameter gradients (the relative-position-bias tables and qkv biases among them) with test_swin_gpu.py's
    tolerances: fp32 3e-4 rel-to-max per gradient, bf16 1.2e-2 on every gradient norm; in bf16 also a cosine of at
    least 0.9995 per gradient."""
    cfg, B = MODELS[model]
    ref, m = make_pair(cfg, compute)
    lo, lr, out, loss = step(ref, m, B, cfg["img_size"])
    check(f"{model}.{compute}.logits", out, lo, 1e-4 if compute == "fp32" else 1e-2)
    assert abs(loss.item() - lr.item()) < (1e-4 if compute == "fp32" else 5e-3)
    names = set()
    worst, cmin = 0.0, 1.0
    for (n, pr), (n2, pm) in zip(ref.named_parameters(), m.named_parameters()):
        assert n == n2 and pm.grad is not None
        names.add(n.rsplit(".", 1)[0].rsplit(".", 1)[-1] + "." + n.rsplit(".", 1)[-1])
        if compute == "fp32":
            worst = max(worst, rel_err(pm.grad, pr.grad))
            assert rel_err(pm.grad, pr.grad) <= 3e-4, f"grad[{n}]"
        else:
            gn_ref, gn = pr.grad.norm().item(), pm.grad.float().norm().item()
            rel = abs(gn - gn_ref) / max(gn_ref, 1e-12)
            worst = max(worst, rel)
            assert rel < 1.2e-2, f"grad-norm[{n}]: {gn:.4g} vs {gn_ref:.4g}"
            if not n.endswith("qkv.bias"):      # its k third is analytically zero: rounding noise on both sides
                c = cosine(pm.grad.float(), pr.grad)
                cmin = min(cmin, c)
                assert c >= 0.9995, f"grad-cosine[{n}]: {c:.6f}"      # measured >= 0.99997
    assert {"attn.relative_position_bias_table", "qkv.bias"} <= names
    print(f"\n  {model}.{compute}: worst grad {'rel-to-max' if compute == 'fp32' else 'norm'} error {worst:.2e}"
          + (f", min cosine {cmin:.6f}" if compute == "bf16" else ""), end="")
