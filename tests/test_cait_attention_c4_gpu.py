"""CaiT's attention kernels against a float64 PyTorch reference (tests/cait_util.py) at the shapes training runs them:
cait_S24_224 at batch 256 (benchmark config C4: N = 196, H = 8, hd = 48, 197 tokens in class attention), the grid
walks those shapes take and the small batches do not, the ViT CLS-only block's interleaved k / v, and determinism.

Error metric: max |got - want| / max |want| over the whole tensor (util.rel_err).  Both sides see the same bf16-rounded
operands.  Bounds, from the kernels' arithmetic, each 2-3x the largest value measured on an MI355X (in brackets; every
test prints its errors beside their bounds with -s):
  * fp32-grade, FP32 = 3e-6: the fp32 kernels compute and store in fp32 [class attention 1.3e-6, softmax 6.5e-7,
    batched GEMM 4.8e-7]; the class-attention softmax that the forward saves for the backward is fp32 in both dtypes
    [7.8e-7].  dbw in bf16, DBW = 8e-7: an fp32 sum of the fp32 dP' rows, no bf16 operand on its path [2.8e-7].
  * One bf16 rounding at the store of an fp32-grade value, at most 2^-8 = 3.9e-3 of the element, VEC = 8e-3: the class
    attention kernels in bf16 [3.3e-3], the batched GEMM's scores and P'v [2.4e-3], and the three-call softmax forward's
    P and P' [3.6e-3].
  * The fused talking-heads kernels keep S, P and P' as bf16 between their phases (LDS planes, MFMA operands), so O
    carries three roundings of the score path on top of its own store [5.8e-3]; the backward adds bf16 dS' and dP'
    operands [9.2e-3]: TH_OUT = 1.5e-2, TH_DQKV = 2.5e-2.  dWl and dWw are fp32 sums over 256 x 8 x 196 x 196 products
    of those bf16-rounded operands, whose errors largely cancel [4.3e-3]: TH_DW = 1e-2.
  * The three-call softmax backward in bf16: dS from bf16 P and dP' through an fp32 row, rounded once at the store
    [3.2e-3]; dWl and dWw from MFMA tiles on bf16 dS' or from per-lane fp32 FMAs [3.5e-3]: SM_DS = SM_DW = 8e-3.
  * Peaked rows (softmax nearly one-hot, scores up to ~60): a bf16 score near 60 is rounded by up to 0.125, which moves
    its exponential by up to 13%; the three-call form stores the same bf16 scores [O 3.9e-2, dq / dk / dv 6.0e-2,
    dWl / dWw 5.1e-2]: PEAK_OUT = 1e-1, PEAK_DQKV = 1.5e-1, PEAK_DW = 1.2e-1.
  * One image of 256 moves dWl, dWw and dbw by at least 2.1e-2 of their largest element (fused and three-call forms):
    at least 2.3x TH_DW and 2.6x SM_DW, so every test at B = 256 also asserts (>= 2x) that a lost image partial would
    be caught.

Walks are checked by invariants instead of a float64 reference per batch size (the B = 256 cases anchor the values): an
image's result from a launch of B images must equal, bit for bit, its result from a launch of that image alone, since the
walk changes neither the operands nor the order of any accumulation.
"""
import pytest
import torch
import torch.nn.functional as F

from cait_util import torch_class_attention, torch_talking_heads, torch_th_softmax
from util import bf16_round, rel_err

pytestmark = pytest.mark.gpu

F64, bt = torch.float64, torch.bfloat16
H8, HD, N196, NSB = 8, 48, 196, 224      # cait_S24_224's attention; NSB: the fused backward writes all 224 key slots
FP32, DBW = 3e-6, 8e-7
VEC = 8e-3
TH_OUT, TH_DQKV, TH_DW = 1.5e-2, 2.5e-2, 1e-2
SM_DS, SM_DW = 8e-3, 8e-3
PEAK_OUT, PEAK_DQKV, PEAK_DW = 1e-1, 1.5e-1, 1.2e-1


@pytest.fixture(scope="module")
def ops(lib):
    from vit_torch_amd import ops as _o
    return _o


def gen(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed)) * scale


def nan(shape, dt):
    return torch.full(shape, float("nan"), device="cuda", dtype=dt)


def check(name, got, want, bound):
    """rel-to-max error, printed beside its bound before it is asserted."""
    g = got.detach().float().cpu()
    assert tuple(g.shape) == tuple(want.shape), f"{name}: shape {tuple(g.shape)} vs {tuple(want.shape)}"
    assert torch.isfinite(g).all(), f"{name}: non-finite values in result"
    e = rel_err(got.detach().double().cpu(), want.double())
    print(f"\n  {name}: {e:.2e} (bound {bound:.1e})", end="")
    assert e <= bound, f"{name}: rel-to-max error {e:.3e} > {bound:.1e}"
    return e


class Acc:
    """rel-to-max error of a tensor compared chunk by chunk: max |got - want| and max |want| over all chunks."""

    def __init__(self):
        self.num, self.den = 0.0, 0.0

    def add(self, name, got, want):
        g = got.detach().double().cpu()
        assert torch.isfinite(g).all(), f"{name}: non-finite values in result"
        self.num = max(self.num, (g - want.double()).abs().max().item())
        self.den = max(self.den, want.abs().max().item())

    def check(self, name, bound):
        e = self.num / self.den
        print(f"\n  {name}: {e:.2e} (bound {bound:.1e})", end="")
        assert e <= bound, f"{name}: rel-to-max error {e:.3e} > {bound:.1e}"
        return e


def margin(name, img, total, bound):
    """The smallest effect of one image on a batch sum (max |its contribution| / max |sum|) against the bound."""
    drop = (img.abs().flatten(1).amax(1) / total.abs().max()).min().item()
    print(f"\n  {name}: one dropped image moves it by >= {drop:.2e} ({drop / bound:.1f}x its bound {bound:.1e})", end="")
    return drop


def bits(t):
    return t.view(torch.int16) if t.dtype == bt else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------ fused talking heads ---
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def fwd_nblk(B, N, cu):
    """query blocks of 32 rows per forward workgroup (vitmi_th_attn_fwd's host formula)."""
    nqb = -(-N // 32)
    return min(max(B * nqb // cu, 1), nqb)


def fwd_batch(nblk, N, cu):
    """a batch whose forward walks `nblk` blocks: the smallest such (the largest for nblk 1)."""
    nqb = -(-N // 32)
    B = -(-2 * cu // nqb) - 1 if nblk == 1 else -(-nblk * cu // nqb)
    assert fwd_nblk(B, N, cu) == nblk and B >= 1
    return B


def walks(nblk, N):
    nqb = -(-N // 32)
    return [min(nblk, nqb - s) for s in range(0, nqb, nblk)]


def th_params(seed, H=H8):
    g = torch.Generator("cpu").manual_seed(seed)
    eye = torch.eye(H)
    Wl = eye + 0.3 * torch.randn(H, H, generator=g)
    Ww = eye + 0.3 * torch.randn(H, H, generator=g)
    bl, bw = 0.2 * torch.randn(H, generator=g), 0.05 * torch.randn(H, generator=g)
    return Wl, bl, Ww, bw


def th_inputs(B, N, seed, scale=0.7):
    """bf16 qkv [B,N,3,H,hd] and dO [B,N,H,hd] on the CPU, plus the mixing parameters."""
    qkv = (gen((B, N, 3, H8, HD), seed) * scale).to(bt)
    dO = gen((B, N, H8, HD), seed + 1).to(bt)
    return qkv, dO, th_params(seed + 2)


def th_fwd(ops, Q, W, B, N):
    O = nan((B, N, H8, HD), bt)
    ops.th_attn_fwd(Q, *W, O, B, H8, N, HD, HD ** -0.5)
    return O


TAIL = 4096


def th_bwd(ops, Q, dO, W, B, N):
    """dqkv [B*N, 3D] (a view of a buffer with a sentinel tail, checked untouched), dS, P', [dWl, dbl, dWw, dbw]."""
    D3 = 3 * H8 * HD
    buf = nan((B * N * D3 + TAIL,), bt)
    buf[B * N * D3:] = 3.0
    dqkv = buf[:B * N * D3].view(B * N, D3)
    dS, Pm = nan((B, H8, N, NSB), bt), nan((B, H8, N, NSB), bt)
    gr = [nan((H8, H8), torch.float32), nan((H8,), torch.float32), nan((H8, H8), torch.float32), nan((H8,), torch.float32)]
    ops.th_attn_bwd(Q, dO, *W, dqkv, dS, Pm, NSB, *gr, B, H8, N, HD, HD ** -0.5)
    torch.cuda.synchronize()
    assert (buf[B * N * D3:] == 3.0).all(), "th_attn_bwd wrote past the end of dqkv"
    return dqkv.view(B, N, 3, H8, HD), dS, Pm, gr


def fused_against_float64(ops, tag, qkv, dO, W, b_out, b_dqkv, b_dw, images_per_chunk=16):
    B, N = qkv.shape[:2]
    r = torch_talking_heads(qkv, dO, *W, HD ** -0.5, F64, images_per_chunk)
    Wd = [t.cuda().contiguous() for t in W]
    Q, dOd = qkv.cuda().contiguous(), dO.cuda().contiguous()
    O = th_fwd(ops, Q, Wd, B, N)
    dqkv, _, _, (dWl, dbl, dWw, dbw) = th_bwd(ops, Q, dOd, Wd, B, N)
    check(f"{tag}.O", O.view(B, N, H8 * HD), r.out, b_out)
    for i, nm in enumerate("qkv"):
        check(f"{tag}.d{nm}", dqkv[:, :, i], r.dqkv[:, :, i], b_dqkv)
    check(f"{tag}.dWl", dWl, r.dWl, b_dw)
    check(f"{tag}.dWw", dWw, r.dWw, b_dw)
    check(f"{tag}.dbw", dbw, r.dbw, DBW)
    # d bl is analytically zero (softmax ignores a per-row constant); the kernel writes zeros
    assert dbl.abs().max().item() == 0.0 and r.dbl.abs().max().item() < 1e-9 * r.dWl.abs().max().item()
    return r


def test_fused_talking_heads_at_c4_against_float64(ops):
    """B = 256, N = 196: the forward walks all 7 query blocks of an image per workgroup (on 256 CUs), the backward fills
    32 whole rows of 8 images.  One image's contribution to dWl, dWw and dbw is at least 2x the bound on each, so a lost
    image partial is caught."""
    B, N = 256, N196
    qkv, dO, W = th_inputs(B, N, 1)
    print(f"\n  C4: forward nblk {fwd_nblk(B, N, cus())} on {cus()} CUs", end="")
    r = fused_against_float64(ops, "c4", qkv, dO, W, TH_OUT, TH_DQKV, TH_DW)
    assert margin("c4.dWl", r.img_dWl, r.dWl, TH_DW) >= 2 * TH_DW
    assert margin("c4.dWw", r.img_dWw, r.dWw, TH_DW) >= 2 * TH_DW
    assert margin("c4.dbw", r.img_dbw, r.dbw, DBW) >= 2 * DBW


def test_fused_talking_heads_max_on_the_last_key(ops):
    """Every row's largest mixed score (and most of its softmax mass) on key N - 1 = 195, the last real key before the
    masked slots 196..223, at a batch whose forward walks 2 blocks per workgroup with a tail of 1."""
    cu = cus()
    B, N = fwd_batch(2, N196, cu), N196
    g = torch.Generator("cpu").manual_seed(5)
    u = torch.randn(1, 1, H8, HD, generator=g) * 0.5
    x = torch.randn(B, N, 3, H8, HD, generator=g) * 0.5
    x[:, :, 0] += u                                   # every query leans on u ...
    x[:, N - 1, 1] = 4.0 * u[0, 0]                    # ... and so does the last key, strongly
    qkv = x.to(bt)
    dO = gen((B, N, H8, HD), 6).to(bt)
    Wl, bl, Ww, bw = th_params(7)
    Wl = torch.eye(H8) + 0.1 * gen((H8, H8), 8)       # proj_l rows sum to about 1: the mix keeps key N - 1 on top
    W = (Wl, bl, Ww, bw)
    q = qkv[:8].float()[:, :, 0].permute(0, 2, 1, 3) * HD ** -0.5
    S = q @ qkv[:8].float()[:, :, 1].permute(0, 2, 3, 1)
    Sm = (S.permute(0, 2, 3, 1) @ Wl.t() + bl).permute(0, 3, 1, 2)
    assert (Sm.argmax(-1) == N - 1).float().mean().item() == 1.0
    fused_against_float64(ops, f"lastkey.B{B}", qkv, dO, W, TH_OUT, TH_DQKV, TH_DW)


def test_fused_talking_heads_peaked_rows(ops):
    """qkv scaled 5x: scores up to ~60, softmax rows nearly one-hot (median row maximum of P about 0.97)."""
    B, N = 8, N196
    qkv, dO, W = th_inputs(B, N, 11, scale=3.5)
    q = qkv[:1].double()[:, :, 0].permute(0, 2, 1, 3) * HD ** -0.5
    P = ((q @ qkv[:1].double()[:, :, 1].permute(0, 2, 3, 1)).permute(0, 2, 3, 1) @ W[0].double().t()
         + W[1].double()).permute(0, 3, 1, 2).softmax(-1)
    print(f"\n  peaked: median row max of P {P.amax(-1).median().item():.3f}", end="")
    assert P.amax(-1).median().item() > 0.9
    fused_against_float64(ops, "peaked", qkv, dO, W, PEAK_OUT, PEAK_DQKV, PEAK_DW)


def fwd_walk_cases():
    return [("N196", k) for k in range(1, 8)] + [("N100", 3), ("N224", 3)]


@pytest.mark.parametrize("case", fwd_walk_cases(), ids=lambda c: f"{c[0]}-nblk{c[1]}")
def test_fused_forward_walk_matches_single_image_launches(ops, case):
    """The forward at a batch whose workgroups walk nblk query blocks (nblk 1..7 at N = 196 with the tails the host
    formula leaves, e.g. 2, 2, 2, 1 at nblk 2; N = 100 and 224 at nblk 3): every row written, and first / last / inner
    images equal to the bit to a launch of that image alone (one block per workgroup)."""
    cu = cus()
    N, nblk = int(case[0][1:]), case[1]
    B = fwd_batch(nblk, N, cu)
    g = torch.Generator(device="cuda").manual_seed(B)
    Q = (torch.randn((B, N, 3, H8, HD), device="cuda", generator=g) * 0.7).to(bt)
    W = [t.cuda() for t in th_params(B)]
    O = th_fwd(ops, Q, W, B, N)
    torch.cuda.synchronize()
    print(f"\n  forward N {N} B {B}: nblk {nblk}, walks {walks(nblk, N)}", end="")
    assert torch.isfinite(O.float()).all(), "rows left unwritten"
    for b in sorted({0, 1, B // 2, B - 2, B - 1}):
        O1 = th_fwd(ops, Q[b:b + 1].contiguous(), W, 1, N)
        assert same_bits(O[b:b + 1], O1), f"image {b}: walked forward differs from a single-image launch"


@pytest.mark.parametrize("B", [13, 255])
def test_fused_backward_matches_single_image_launches(ops, B):
    """The backward's XCD map pads the grid to whole rows of 8 images; at 13 and 255 the last row is part-filled.  dq, dk
    and dv of sampled images (the first and last of an XCD row, the last image) equal a single-image launch to the bit;
    the parameter gradients are finite; nothing is written past dqkv."""
    N = N196
    g = torch.Generator(device="cuda").manual_seed(100 + B)
    Q = (torch.randn((B, N, 3, H8, HD), device="cuda", generator=g) * 0.7).to(bt)
    dO = torch.randn((B, N, H8, HD), device="cuda", generator=g).to(bt)
    W = [t.cuda() for t in th_params(B)]
    dqkv, _, _, gr = th_bwd(ops, Q, dO, W, B, N)
    assert torch.isfinite(dqkv.float()).all() and all(torch.isfinite(t).all() for t in gr)
    for b in sorted({0, 7, 8, B // 2, B - 1}):
        d1, _, _, _ = th_bwd(ops, Q[b:b + 1].contiguous(), dO[b:b + 1].contiguous(), W, 1, N)
        assert same_bits(dqkv[b:b + 1], d1), f"image {b}: batched backward differs from a single-image launch"


# --------------------------------------------------------------------------- three-call softmax at C4 rows ---
# (B, H, N, ld): B * N rows; the backward's grid stops at 512 workgroups of 4 rows, so past 2048 rows each walks several
SM_CASES = {
    "c4_h8": (256, 8, 196, 200),          # 50176 rows: ~98 row groups per workgroup
    "c4_h4": (256, 4, 196, 200),          # cait_XXS24_224
    "b11": (11, 8, 196, 200),             # 2156 rows: just past the cap, uneven walk
    "ld198": (11, 8, 197, 198),           # ld % 4 != 0: the non-vector kernels
}
SM_PARAMS = [(c, f) for c in SM_CASES for f in ("mfma", "fma", "fp32") if not (c == "ld198" and f == "mfma")]


@pytest.mark.parametrize("case,form", SM_PARAMS, ids=[f"{c}-{f}" for c, f in SM_PARAMS])
def test_th_softmax_at_c4_rows(ops, lib, case, form):
    """th_softmax_fwd / _bwd on random score rows (pad columns NaN): P, P', dS and the four parameter gradients against
    float64, chunk by chunk; dS of sampled images equal to a single-image launch to the bit.  bf16 in both gradient
    forms (MFMA tiles / per-lane FMAs), and fp32."""
    B, H, N, ld = SM_CASES[case]
    dt = torch.float32 if form == "fp32" else bt
    lib.vitmi_debug_th_mfma(1 if form == "mfma" else 0)
    rd = (lambda t: t) if dt == torch.float32 else bf16_round
    S = rd(gen((B, H, N, N), 20 + B))
    dPm = rd(gen((B, H, N, N), 21 + B))
    W = th_params(22 + H, H)
    Wl, bl, Ww, bw = (t * 0.5 if t.dim() == 2 else t for t in W)
    pad = lambda t: F.pad(t, (0, ld - N), value=float("nan")).to("cuda", dt).contiguous()
    Sd, dPd = pad(S), pad(dPm)
    Wd = [t.cuda() for t in (Wl, bl, Ww, bw)]
    P, Pm = nan((B, H, N, ld), dt), nan((B, H, N, ld), dt)
    ops.th_softmax_fwd(Sd, *Wd, P, Pm, B, H, N, N, ld)
    dS = nan((B, H, N, ld), dt)
    g = [nan((H * H,), torch.float32), nan((H,), torch.float32), nan((H * H,), torch.float32), nan((H,), torch.float32)]
    ops.th_softmax_bwd(Sd, P, dPd, Wd[0], Wd[2], dS, *g, B, H, N, N, ld)
    torch.cuda.synchronize()
    acc = {k: Acc() for k in ("P", "Pm", "dS")}
    gsum = [torch.zeros(H, H, dtype=F64), torch.zeros(H, dtype=F64), torch.zeros(H, H, dtype=F64), torch.zeros(H, dtype=F64)]
    img = ([], [], [])
    step = 16
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        r = torch_th_softmax(S[b0:b1], dPm[b0:b1], Wl, bl, Ww, bw)
        acc["P"].add("P", P[b0:b1, ..., :N], r[0])
        acc["Pm"].add("Pm", Pm[b0:b1, ..., :N], r[1])
        acc["dS"].add("dS", dS[b0:b1, ..., :N], r[2])
        for t, x in zip(gsum, r[3:7]):
            t += x
        for lst, x in zip(img, r[7:]):
            lst.append(x)
    fp = dt == torch.float32
    tag = f"softmax.{case}.{form}"
    acc["P"].check(f"{tag}.P", FP32 if fp else VEC)
    acc["Pm"].check(f"{tag}.Pm", FP32 if fp else VEC)
    acc["dS"].check(f"{tag}.dS", FP32 if fp else SM_DS)
    bw_ = FP32 if fp else SM_DW
    check(f"{tag}.dWl", g[0].view(H, H), gsum[0], bw_)
    check(f"{tag}.dWw", g[2].view(H, H), gsum[2], bw_)
    check(f"{tag}.dbw", g[3], gsum[3], FP32 if fp else DBW)
    # d bl is analytically zero: rounding noise only, bounded against the scale of dWl
    assert g[1].abs().max().item() <= (1e-5 if fp else 2e-2) * gsum[0].abs().max().item()
    if B >= 32:
        for nm, i, t, bd in (("dWl", 0, gsum[0], bw_), ("dWw", 1, gsum[2], bw_), ("dbw", 2, gsum[3], FP32 if fp else DBW)):
            assert margin(f"{tag}.{nm}", torch.cat(img[i]), t, bd) >= 2 * bd
    for b in sorted({0, 1, B // 2, B - 1}):
        one = lambda t: t[b:b + 1].contiguous()
        dS1 = nan((1, H, N, ld), dt)
        g1 = [nan((H * H,), torch.float32), nan((H,), torch.float32), nan((H * H,), torch.float32), nan((H,), torch.float32)]
        ops.th_softmax_bwd(one(Sd), one(P), one(dPd), Wd[0], Wd[2], dS1, *g1, 1, H, N, N, ld)
        assert same_bits(dS[b:b + 1, ..., :N], dS1[..., :N]), f"image {b}: dS differs from a single-image launch"


# ----------------------------------------------------------------------------- three-call products at C4 ---
@pytest.mark.parametrize("dt", [bt, torch.float32], ids=["bf16", "fp32"])
def test_batched_gemm_scores_and_pv_at_c4(ops, dt):
    """The three-call form's two forward products at batch B * H = 2048, reading q, k and v in place from the
    [B, N, 3, H, hd] qkv: scale q k^T into [B, H, N, 200] (pad columns left untouched), and P'v from score rows whose pad
    columns hold NaN."""
    B, N, H, hd = 256, N196, H8, HD
    NS, D, D3 = 200, H * hd, 3 * H * hd
    scale = hd ** -0.5
    rd = (lambda t: t) if dt == torch.float32 else bf16_round
    qkv = rd(gen((B, N, D3), 30))
    Q = qkv.to("cuda", dt)
    S = nan((B, H, N, NS), dt)
    ops.gemm_batched(Q, Q, S, M=N, N=N, K=hd, lda=D3, ldb=D3, ldc=NS, a_kmajor=True, b_kmajor=True,
                     batch=B * H, batch_inner=H, a_bs=(N * D3, hd), b_bs=(N * D3, hd), c_bs=(H * N * NS, N * NS),
                     b_off=H * hd, alpha=scale)
    Pm = rd(gen((B, H, N, N), 31).softmax(-1) * 1.3 - 0.1 / N)          # P' = proj_w(P): rows need not sum to one
    Pd = F.pad(Pm, (0, NS - N), value=float("nan")).to("cuda", dt).contiguous()
    O = nan((B, N, D), dt)
    ops.gemm_batched(Pd, Q, O, M=N, N=hd, K=N, lda=NS, ldb=D3, ldc=D, a_kmajor=True, b_kmajor=False,
                     batch=B * H, batch_inner=H, a_bs=(H * N * NS, N * NS), b_bs=(N * D3, hd), c_bs=(N * D, hd),
                     b_off=2 * D)
    torch.cuda.synchronize()
    assert S[..., N:].isnan().all(), "pad columns of the scores were written"
    a_s, a_o = Acc(), Acc()
    for b0 in range(0, B, 32):
        x = qkv[b0:b0 + 32].to(F64).view(-1, N, 3, H, hd).permute(2, 0, 3, 1, 4)
        a_s.add("S", S[b0:b0 + 32, ..., :N], (x[0] @ x[1].transpose(-2, -1)) * scale)
        a_o.add("O", O[b0:b0 + 32], (Pm[b0:b0 + 32].to(F64) @ x[2]).transpose(1, 2).reshape(-1, N, D))
    tag = f"gemm_batched.{'fp32' if dt == torch.float32 else 'bf16'}"
    a_s.check(f"{tag}.scores", FP32 if dt == torch.float32 else VEC)
    a_o.check(f"{tag}.PV", FP32 if dt == torch.float32 else VEC)


# ------------------------------------------------------------------------------------------ class attention ---
# (B, H, N, hd, token stride in units of D, dtype): stride 1 = CaiT's separate k and v, 2 = the ViT CLS-only block's
# interleaved kv rows [k | v]
CA_CASES = {
    "cait_c4": (256, 8, 197, 48, 1, bt),
    "vit_b16_cls": (256, 12, 197, 64, 2, bt),
    "c3_cls": (128, 12, 145, 64, 2, bt),
    "c1_cls": (128, 6, 5, 64, 2, bt),                 # dino_vits16 at 32 x 32 (C1): B * H = 768, whole workgroups
    "idle_waves": (127, 6, 5, 64, 2, bt),             # B * H = 762: the last workgroup runs 2 of its 4 waves
    "scalar_hd12": (256, 8, 197, 12, 1, bt),          # hd % 8 != 0: the element-wise bf16 kernel
    "fp32_c4": (256, 8, 197, 48, 1, torch.float32),
    "fp32_cls": (256, 12, 197, 64, 2, torch.float32),
}


def class_attention(ops, q, kv, do, B, H, N, hd, st, dt):
    """forward + backward on the device, outputs NaN-filled: (out, p_save, dq, dk, dv) with dk / dv views of one
    [B * N, st * D] buffer (st 2: interleaved, both halves written)."""
    D = H * hd
    Q, KV, DO = q.to("cuda", dt).contiguous(), kv.to("cuda", dt).contiguous(), do.to("cuda", dt).contiguous()
    k, v = (KV, KV[:, D:]) if st == 2 else (KV[:, :D].contiguous(), KV[:, D:].contiguous())
    out, ps = nan((B, D), dt), nan((B * H * N,), torch.float32)
    ops.class_attn_fwd(Q, k, v, st * D, out, ps, B, H, N, hd, hd ** -0.5)
    dq = nan((B, D), dt)
    if st == 2:
        dkv = nan((B * N, 2 * D), dt)
        dk, dv = dkv, dkv[:, D:]
    else:
        dk, dv = nan((B * N, D), dt), nan((B * N, D), dt)
    ops.class_attn_bwd(Q, k, v, st * D, DO, ps, dq, dk, dv, st * D, B, H, N, hd, hd ** -0.5)
    torch.cuda.synchronize()
    if st == 2:
        assert torch.isfinite(dkv.float()).all()
        dk, dv = dkv[:, :D], dkv[:, D:]
    return out, ps, dq, dk.reshape(B, N, D), dv.reshape(B, N, D)


def ca_inputs(B, H, N, hd, dt, seed):
    D = H * hd
    rd = (lambda t: t) if dt == torch.float32 else bf16_round
    return rd(gen((B, D), seed)), rd(gen((B * N, 2 * D), seed + 1)), rd(gen((B, D), seed + 2))


@pytest.mark.parametrize("case", list(CA_CASES))
def test_class_attention_at_training_shapes(ops, case):
    B, H, N, hd, st, dt = CA_CASES[case]
    D = H * hd
    q, kv, do = ca_inputs(B, H, N, hd, dt, 40)
    kr, vr = kv.view(B, N, 2 * D)[..., :D], kv.view(B, N, 2 * D)[..., D:]
    r = torch_class_attention(q, kr, vr, do, H)
    got = class_attention(ops, q, kv, do, B, H, N, hd, st, dt)
    bound = FP32 if dt == torch.float32 else VEC
    tag = f"class_attn.{case}"
    check(f"{tag}.out", got[0], r[0], bound)
    check(f"{tag}.p", got[1].view(B, H, N), r[1], FP32)
    for nm, x, w in zip(("dq", "dk", "dv"), got[2:], r[2:]):
        check(f"{tag}.{nm}", x, w, bound)


# ------------------------------------------------------------------------------------------------ determinism ---
def test_c4_kernels_are_deterministic(ops):
    """At C4, five runs of each kernel give the same bits: th_attn_fwd; th_attn_bwd with its parameter gradients;
    th_softmax_bwd with its parameter gradients; class attention forward and backward."""
    B, N, H, D = 256, N196, H8, H8 * HD
    g = torch.Generator(device="cuda").manual_seed(50)
    Q = (torch.randn((B, N, 3, H, HD), device="cuda", generator=g) * 0.7).to(bt)
    dO = torch.randn((B, N, H, HD), device="cuda", generator=g).to(bt)
    W = [t.cuda() for t in th_params(50)]

    def fused():
        O = th_fwd(ops, Q, W, B, N)
        dqkv, dS, Pm, gr = th_bwd(ops, Q, dO, W, B, N)
        return [O, dqkv, dS, Pm] + gr

    ld = 200
    S = torch.randn((B, H, N, ld), device="cuda", generator=g).to(bt)
    dPm = torch.randn((B, H, N, ld), device="cuda", generator=g).to(bt)
    P, Pm = nan((B, H, N, ld), bt), nan((B, H, N, ld), bt)
    ops.th_softmax_fwd(S, *W, P, Pm, B, H, N, N, ld)

    def softmax_bwd():
        dS = nan((B, H, N, ld), bt)
        gr = [nan((H * H,), torch.float32), nan((H,), torch.float32), nan((H * H,), torch.float32), nan((H,), torch.float32)]
        ops.th_softmax_bwd(S, P, dPm, W[0], W[2], dS, *gr, B, H, N, N, ld)
        return [dS[..., :N]] + gr

    q, kv, do = ca_inputs(B, H, N + 1, HD, bt, 51)

    def cls():
        return list(class_attention(ops, q, kv, do, B, H, N + 1, HD, 1, bt))

    for name, fn in (("fused talking heads", fused), ("th_softmax_bwd", softmax_bwd), ("class attention", cls)):
        first = [t.clone() for t in fn()]
        for rep in range(4):
            again = fn()
            for i, (a, b) in enumerate(zip(first, again)):
                assert same_bits(a, b), f"{name}: output {i} differs on repeat {rep + 1}"
        print(f"\n  {name}: 5 runs, identical bits", end="")
