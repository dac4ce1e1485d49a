"""Window-12 Swin (windows of 65..144 tokens) on the HIP path: the window-attention and relative-position kernels
against PyTorch, determinism, and window-12 models against the CPU oracle (oracle/swin_ref.py, generic in the
window size)."""
import pytest
import torch
import torch.nn.functional as F

from swin_util import torch_window_attention
from util import assert_close, bf16_round

pytestmark = pytest.mark.gpu


def gen(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed)) * scale


@pytest.fixture(scope="module")
def ops(lib):
    from vit_torch_amd import ops as _o
    return _o


CASES = [(2, 24, 24, 12, 0, 2, 32), (1, 24, 24, 12, 6, 3, 32), (2, 12, 12, 12, 0, 4, 32), (1, 24, 24, 12, 6, 2, 16),
         (1, 24, 24, 12, 0, 2, 24), (1, 24, 24, 12, 6, 2, 64), (1, 18, 18, 9, 4, 2, 32), (1, 20, 20, 10, 5, 2, 32),
         (1, 22, 22, 11, 0, 3, 32)]


@pytest.mark.parametrize("mfma", [True, False])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,Hh,Ww,ws,shift,H,hd", CASES)
def test_window12_attention_in_token_order(ops, lib, mfma, dt, B, Hh, Ww, ws, shift, H, hd):
    if not mfma:
        lib.vitmi_debug_win_attn_mfma(0)               # the fp32 vector kernels for every shape
    C, N, L = H * hd, ws * ws, Hh * Ww
    scale = hd ** -0.5
    rd = bf16_round if dt == torch.bfloat16 else (lambda t: t)
    qkv = rd(gen((B, L, 3 * C), 1))
    do = rd(gen((B, L, C), 2))
    bias = gen((H, N, N), 3, 0.5)
    o, mask, dq_ref, db_ref = torch_window_attention(qkv, do, bias, B, Hh, Ww, ws, shift, H, hd)[:4]
    Bw = B * (Hh // ws) * (Ww // ws)
    Q = qkv.to("cuda", dt).contiguous()
    O = torch.full((B, L, C), float("nan"), device="cuda").to(dt)
    lse = torch.empty(Bw * H * N, device="cuda")
    bd = bias.cuda().contiguous()
    md = mask.cuda().contiguous() if mask is not None else None
    ops.win_attn_fwd(Q, O, lse, bd, md, Bw, H, N, hd, Hh, Ww, ws, shift, scale)
    assert_close("win12.out", O, o, 2e-5 if dt == torch.float32 else 1.5e-2)
    dqkv = torch.full((B, L, 3 * C), float("nan"), device="cuda").to(dt)
    dbias = torch.full((H * N * N,), float("nan"), device="cuda")
    ops.win_attn_bwd(Q, do.to("cuda", dt).contiguous(), lse, bd, md, dqkv, dbias, Bw, H, N, hd, Hh, Ww, ws, shift, scale)
    bt = 5e-5 if dt == torch.float32 else 2.5e-2
    assert_close("win12.dqkv", dqkv, dq_ref, bt)
    assert_close("win12.dbias", dbias.view(H, N, N), db_ref, bt)
    if ops.win_attn_bwd_fuses_qkv_bias(Q, hd):
        dqkv2 = torch.empty_like(dqkv)
        qb = torch.full((3 * C,), float("nan"), device="cuda")
        ops.win_attn_bwd(Q, do.to("cuda", dt).contiguous(), lse, bd, md, dqkv2, dbias, Bw, H, N, hd, Hh, Ww, ws, shift,
                         scale, dqkv_bias=qb)
        assert torch.equal(dqkv2, dqkv)
        assert_close("win12.dqkv_bias", qb, dq_ref.reshape(-1, 3 * C).sum(0), 2.5e-2)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_window12_walk_of_many_windows(ops, dt):
    """More windows than backward workgroups per head (the MFMA kernel in bf16, the vector kernels in fp32): a
    workgroup walks several windows and its d(bias) partial and qkv-bias sums accumulate across the walk."""
    B, Hh, Ww, ws, shift, H, hd = 3, 48, 48, 12, 6, 8, 32    # 48 windows, 8 heads: 32 workgroups per head
    C, N, L = H * hd, ws * ws, Hh * Ww
    scale = hd ** -0.5
    qkv = bf16_round(gen((B, L, 3 * C), 11))
    do = bf16_round(gen((B, L, C), 12))
    bias = gen((H, N, N), 13, 0.5)
    o, mask, dq_ref, db_ref = torch_window_attention(qkv, do, bias, B, Hh, Ww, ws, shift, H, hd)[:4]
    Bw = B * (Hh // ws) * (Ww // ws)
    Q = qkv.to("cuda", dt).contiguous()
    O = torch.empty((B, L, C), device="cuda", dtype=dt)
    lse = torch.empty(Bw * H * N, device="cuda")
    bd, md = bias.cuda().contiguous(), mask.cuda().contiguous()
    ops.win_attn_fwd(Q, O, lse, bd, md, Bw, H, N, hd, Hh, Ww, ws, shift, scale)
    tf, tb = (1.5e-2, 2.5e-2) if dt == torch.bfloat16 else (2e-5, 5e-5)
    assert_close("walk.out", O, o, tf)
    dqkv = torch.empty((B, L, 3 * C), device="cuda", dtype=dt)
    dbias = torch.empty(H * N * N, device="cuda")
    fuse = ops.win_attn_bwd_fuses_qkv_bias(Q, hd)
    qb = torch.full((3 * C,), float("nan"), device="cuda") if fuse else None
    ops.win_attn_bwd(Q, do.to("cuda", dt).contiguous(), lse, bd, md, dqkv, dbias, Bw, H, N, hd, Hh, Ww,
                     ws, shift, scale, dqkv_bias=qb)
    assert_close("walk.dqkv", dqkv, dq_ref, tb)
    assert_close("walk.dbias", dbias.view(H, N, N), db_ref, tb)
    if fuse:
        assert_close("walk.dqkv_bias", qb, dq_ref.reshape(-1, 3 * C).sum(0), 2.5e-2)


def test_window13_is_refused_with_the_limit(ops):
    from vit_torch_amd._lib import VitmiError
    ws, H, hd = 13, 1, 32
    N, Hh = ws * ws, 13
    qkv = torch.zeros((1, Hh * Hh, 3 * H * hd), device="cuda", dtype=torch.bfloat16)
    O = torch.empty((1, Hh * Hh, H * hd), device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(H * N, device="cuda")
    bias = torch.zeros(H * N * N, device="cuda")
    with pytest.raises(VitmiError, match="144"):
        ops.win_attn_fwd(qkv, O, lse, bias, None, 1, H, N, hd, Hh, Hh, ws, 0, hd ** -0.5)


@pytest.mark.parametrize("mfma", [True, False])
def test_window12_kernels_are_deterministic(ops, lib, mfma):
    if not mfma:
        lib.vitmi_debug_win_attn_mfma(0)
    B, Hh, Ww, ws, shift, H, hd = 2, 36, 36, 12, 6, 4, 32
    C, N, L = H * hd, ws * ws, Hh * Ww
    Bw = B * (Hh // ws) * (Ww // ws)
    scale = hd ** -0.5
    from oracle.swin_ref import shift_attn_mask
    Q = gen((B, L, 3 * C), 21).to("cuda", torch.bfloat16)
    dO = gen((B, L, C), 22).to("cuda", torch.bfloat16)
    bd = gen((H, N, N), 23, 0.5).cuda().contiguous()
    md = shift_attn_mask(Hh, Ww, ws, shift).cuda().contiguous()
    fuse = ops.win_attn_bwd_fuses_qkv_bias(Q, hd)
    runs = []
    for _ in range(3):
        O = torch.empty((B, L, C), device="cuda", dtype=torch.bfloat16)
        lse = torch.empty(Bw * H * N, device="cuda")
        ops.win_attn_fwd(Q, O, lse, bd, md, Bw, H, N, hd, Hh, Ww, ws, shift, scale)
        dqkv = torch.empty((B, L, 3 * C), device="cuda", dtype=torch.bfloat16)
        dbias = torch.empty(H * N * N, device="cuda")
        qb = torch.empty(3 * C, device="cuda") if fuse else None
        ops.win_attn_bwd(Q, dO, lse, bd, md, dqkv, dbias, Bw, H, N, hd, Hh, Ww, ws, shift, scale, dqkv_bias=qb)
        runs.append([t.clone() for t in (O, lse, dqkv, dbias) + ((qb,) if fuse else ())])
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bfloat16 else a, b.view(torch.uint8) if b.dtype == torch.bfloat16 else b)


def test_window12_relpos_bias_gather_scatter(ops):
    from oracle.swin_ref import relative_position_index
    ws, H = 12, 4
    N, T = ws * ws, (2 * ws - 1) ** 2
    table = gen((T, H), 1)
    idx = relative_position_index(ws)
    want = table[idx.view(-1)].view(N, N, H).permute(2, 0, 1)
    bias = torch.empty(H * N * N, device="cuda")
    ops.relpos_bias_gather(table.cuda(), idx.cuda(), bias, T, H, N)
    assert torch.equal(bias.view(H, N, N).cpu(), want)
    db = gen((H, N, N), 2)
    want_dt = torch.zeros(T, H).index_add_(0, idx.view(-1), db.permute(1, 2, 0).reshape(N * N, H))
    dt = torch.full((T, H), float("nan"), device="cuda")
    ops.relpos_bias_scatter(db.cuda().contiguous(), idx.cuda(), dt, T, H, N)
    assert_close("dtable12", dt, want_dt, 1e-6)
    dt2 = torch.empty_like(dt)
    ops.relpos_bias_scatter(db.cuda().contiguous(), idx.cuda(), dt2, T, H, N)
    assert torch.equal(dt, dt2)


TINY12 = dict(img_size=96, patch_size=4, in_chans=3, num_classes=10, embed_dim=32, depths=[2, 2], num_heads=[1, 2],
              window_size=12, drop_path_rate=0.0)


def make_pair(cfg, compute, residual="fp32", seed=7):
    from oracle.swin_ref import SwinTransformer as Ref
    from oracle.vit_ref import seeded_init_
    from vit_torch_amd import SwinTransformer
    ref = Ref(**cfg)
    seeded_init_(ref, seed)
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


def test_swin_window12_tiny_fp32_matches_oracle():
    ref, m = make_pair(TINY12, "fp32")
    assert m.layers[0].blocks[1].shift_size == 6 and m.layers[1].blocks[1].shift_size == 0
    lo, lr, out, loss = step(ref, m, 2, 96)
    assert_close("logits", out, lo, 1e-4)
    assert abs(loss.item() - lr.item()) < 1e-4
    for (n, pr), (n2, pm) in zip(ref.named_parameters(), m.named_parameters()):
        assert n == n2
        assert_close(f"grad[{n}]", pm.grad, pr.grad, 3e-4)


@pytest.mark.parametrize("residual", ["fp32", "bf16"])
def test_swin_window12_tiny_bf16_close_to_oracle(residual):
    ref, m = make_pair(TINY12, "bf16", residual)
    lo, lr, out, loss = step(ref, m, 4, 96)
    assert_close("logits", out, lo, 1e-2)
    assert abs(loss.item() - lr.item()) < 5e-3
    for (n, pr), (_, pm) in zip(ref.named_parameters(), m.named_parameters()):
        gn_ref, gn = pr.grad.norm().item(), pm.grad.float().norm().item()
        assert abs(gn - gn_ref) / max(gn_ref, 1e-12) < 1.2e-2, f"grad-norm[{n}]: {gn:.4g} vs {gn_ref:.4g}"


def test_swin_window12_graph_replay_equals_the_eager_step():
    from vit_torch_amd import CrossEntropyLoss, FusedSGD, GraphedStep
    _, m0 = make_pair(TINY12, "bf16", "bf16")
    m0.train()
    g = torch.Generator("cpu").manual_seed(0)
    x, y = torch.randn(8, 3, 96, 96, generator=g).cuda(), torch.randint(0, 10, (8,), generator=g).cuda()
    m0.engine()
    o0 = FusedSGD(m0.parameters(), lr=0.0, momentum=0.9)
    with torch.no_grad():
        eager = float(CrossEntropyLoss()(m0(x), y).item())
    gs0 = GraphedStep(m0, CrossEntropyLoss(), o0, x, y)
    assert float(gs0(gs0.x, gs0.y).item()) == pytest.approx(eager, rel=1e-6)


def test_swin_b_384_full_size_fp32_logits_within_1e3():
    """swin_base_patch4_window12_384 (drop-path 0), batch 2, parity mode, against an oracle model with the same
    weights."""
    from oracle.swin_ref import SwinTransformer as Ref
    from oracle.vit_ref import seeded_init_
    from vit_torch_amd import VisionModelZoo
    ref = Ref(img_size=384, patch_size=4, embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32],
              window_size=12, num_classes=10, drop_path_rate=0.0)
    seeded_init_(ref, 9)
    m = VisionModelZoo.get_model("swin_base_patch4_window12_384", pretrained=False, classifier=None,
                                 drop_path_rate=0.0, num_classes=10, compute_dtype="fp32")
    m.load_state_dict(ref.state_dict(), strict=True)
    m = m.cuda()
    lo, lr, out, loss = step(ref, m, 2, 384)
    assert_close("swin-B/384 logits", out, lo, 1e-3)
    assert abs(loss.item() - lr.item()) < 1e-3


def _fixture(name):
    import os
    from fixture_codec import load
    return load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))


def test_window_attention_ws12_fixture(ops):
    """The reference's WindowAttention at window 12 (tests/golden/window_attention_ws12.npz) through the kernels,
    without and with the shift-6 mask.  The fixture's 8 windows are the 2x2 windows of two 24x24 images; the kernels
    take tokens in image order, so the windows are laid back into images first.  The two Linears are plain fp32
    matrix products here: what is under test is the attention and the relative-position bias."""
    from fixture_codec import check, group
    from oracle.swin_ref import window_partition, window_reverse
    f = _fixture("window_attention_ws12")
    ws, H, C = 12, 2, 64
    hd, N, scale = C // H, ws * ws, (C // H) ** -0.5
    Bw = f["x"].shape[0]
    Bi, Hh, Ww = Bw // 4, 24, 24
    st = {k: v.cuda() for k, v in group(f, "state").items()}
    Wq, bq, Wp, bp = st["qkv.weight"], st["qkv.bias"], st["proj.weight"], st["proj.bias"]

    def to_img(t):
        c = t.shape[-1]
        return window_reverse(t.reshape(Bw, ws, ws, c), ws, Hh, Ww).reshape(Bi * Hh * Ww, c).cuda().contiguous()

    def to_win(t, c):
        return window_partition(t.detach().cpu().view(Bi, Hh, Ww, c), ws).reshape(Bw, N, c)

    idx = st["relative_position_index"].contiguous()
    table = st["relative_position_bias_table"].contiguous()
    T = table.shape[0]
    for masked in (False, True):
        sfx = "_masked" if masked else ""
        bias = torch.empty(H * N * N, device="cuda")
        ops.relpos_bias_gather(table, idx, bias, T, H, N)
        mask = f["mask"].cuda().contiguous() if masked else None
        x = to_img(f["x"])
        qkv = (x @ Wq.t() + bq).contiguous()
        O, lse = torch.empty(Bi * Hh * Ww, C, device="cuda"), torch.empty(Bw * H * N, device="cuda")
        ops.win_attn_fwd(qkv, O, lse, bias, mask, Bw, H, N, hd, Hh, Ww, ws, 0, scale)
        y = O @ Wp.t() + bp
        check("y" + sfx, to_win(y, C), f["y" + sfx], 2e-5)
        dy = to_img(f["dy"])
        dO = (dy @ Wp).contiguous()
        dqkv, dbias = torch.empty(Bi * Hh * Ww, 3 * C, device="cuda"), torch.empty(H * N * N, device="cuda")
        ops.win_attn_bwd(qkv, dO, lse, bias, mask, dqkv, dbias, Bw, H, N, hd, Hh, Ww, ws, 0, scale)
        dtable = torch.empty(T, H, device="cuda")
        ops.relpos_bias_scatter(dbias, idx, dtable, T, H, N)
        check("dx" + sfx, to_win(dqkv @ Wq, C), f["dx" + sfx], 1e-4)
        want = group(f, "grad" + sfx)
        check("grad.table" + sfx, dtable, want["relative_position_bias_table"], 1e-4)
        check("grad.qkv.weight" + sfx, dqkv.t() @ x, want["qkv.weight"], 1e-4)
        check("grad.qkv.bias" + sfx, dqkv.sum(0), want["qkv.bias"], 1e-4)
        check("grad.proj.weight" + sfx, dy.t() @ O, want["proj.weight"], 1e-4)


def test_swin_tiny_ws12_fixture_fp32():
    """The reference's two-stage window-12 SwinTransformer (tests/golden/swin_tiny_ws12.npz) on the HIP path; the
    relative-position index and shift mask are the model's own, compared with the reference's."""
    from fixture_codec import check, group
    from vit_torch_amd import CrossEntropyLoss, SwinTransformer
    f = _fixture("swin_tiny_ws12")
    m = SwinTransformer(img_size=96, patch_size=4, in_chans=3, num_classes=10, embed_dim=32, depths=[2, 2],
                        num_heads=[1, 2], window_size=12, drop_path_rate=0.0, compute_dtype="fp32")
    assert torch.equal(m.layers[0].blocks[1].attn_mask.cpu(), f["attn_mask"])
    for layer in m.layers:
        for blk in layer.blocks:
            assert torch.equal(blk.attn.relative_position_index.cpu(), f["relative_position_index"])
    res = m.load_state_dict(group(f, "state"), strict=False)
    assert not res.unexpected_keys and all(k.endswith(("relative_position_index", "attn_mask")) for k in res.missing_keys)
    m = m.cuda()
    out = m(f["x"].cuda())
    loss = CrossEntropyLoss()(out, f["labels"].cuda())
    m.zero_grad(); loss.backward()
    check("logits", out, f["logits"], 1e-4)
    assert abs(loss.item() - f["loss"].item()) < 1e-4
    for n, p in m.named_parameters():
        check(f"grad[{n}]", p.grad, f["grad/" + n], 3e-4)
