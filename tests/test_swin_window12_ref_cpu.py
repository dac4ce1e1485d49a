"""The float64 reference that the window-attention kernel tests trust (swin_util.torch_window_attention), pinned to the
oracle's WindowAttention module at windows 9 and 12, and the arithmetic of test_swin_window12_f64_gpu.py's walk table,
which needs no GPU."""
import pytest
import torch

from swin_util import F64, WALKS12, big_rows, drop_margins, gen, inputs, torch_window_attention, walk_shape
from test_swin_window12_f64_gpu import FP32_GRADE, QKV_BIAS      # that file carries its own measured bounds


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("ws", [9, 12])
def test_reference_equals_the_oracle_window_attention(ws, shift):
    """Two images of 2 x 3 windows, 3 heads of 8, all in float64.  The helper gets the module's own qkv projection
    output, laid out in image order, and d(out) ahead of `proj`; the module runs on the rolled, partitioned windows with
    the shift mask.  out, dqkv and d(relative-position table) (the helper's d(bias) summed through the module's index)
    agree to 1e-12."""
    from oracle.swin_ref import WindowAttention, shift_attn_mask, window_partition, window_reverse
    B, Hh, Ww, H, hd = 2, 2 * ws, 3 * ws, 3, 8
    sh = ws // 2 if shift else 0
    C, N, L = H * hd, ws * ws, Hh * Ww
    torch.manual_seed(ws)
    m = WindowAttention(C, (ws, ws), H).to(F64)
    with torch.no_grad():
        m.relative_position_bias_table.copy_(gen(tuple(m.relative_position_bias_table.shape), 1, 0.5))
    x = gen((B, L, C), 2).to(F64)
    do = gen((B, L, C), 3).to(F64)

    def to_windows(t):
        t = t.view(B, Hh, Ww, -1)
        if sh:
            t = torch.roll(t, shifts=(-sh, -sh), dims=(1, 2))
        return window_partition(t, ws).view(-1, N, t.shape[-1])

    def to_image(t):
        t = window_reverse(t.reshape(-1, ws, ws, t.shape[-1]), ws, Hh, Ww)
        if sh:
            t = torch.roll(t, shifts=(sh, sh), dims=(1, 2))
        return t.reshape(B, L, -1)

    seen = {}

    def keep_qkv(mod, args, output):
        output.retain_grad()
        seen["qkv"] = output

    def keep_proj_input(mod, args):
        seen["pre"] = args[0]

    h1 = m.qkv.register_forward_hook(keep_qkv)
    h2 = m.proj.register_forward_pre_hook(keep_proj_input)
    mask = shift_attn_mask(Hh, Ww, ws, sh).to(F64) if sh else None
    m(to_windows(x), mask)
    h1.remove(); h2.remove()
    seen["pre"].backward(to_windows(do))
    qkv_img = to_image(seen["qkv"].detach())
    idx = m.relative_position_index.view(-1)
    bias = m.relative_position_bias_table.detach()[idx].view(N, N, H).permute(2, 0, 1).contiguous()
    r = torch_window_attention(qkv_img, do, bias, B, Hh, Ww, ws, sh, H, hd, F64, images_per_chunk=1)
    assert (r.mask is None) == (not sh)
    dtable = torch.zeros_like(m.relative_position_bias_table).index_add_(0, idx, r.dbias.permute(1, 2, 0).reshape(N * N, H))
    for name, got, want in (("out", r.out, to_image(seen["pre"].detach())), ("dqkv", r.dqkv, to_image(seen["qkv"].grad)),
                            ("dtable", dtable, m.relative_position_bias_table.grad)):
        assert got.dtype == F64 and want.dtype == F64
        e = ((got - want).abs().max() / want.abs().max()).item()
        assert e <= 1e-12, f"{name}: {e:.3e}"
    # lse in the kernels' layout [Bw, H, N], window bw under mask window bw % nW, from the module's own qkv output
    q, k = seen["qkv"].detach().view(-1, N, 3, H, hd).permute(2, 0, 3, 1, 4)[:2]
    s = (q * hd ** -0.5) @ k.transpose(-2, -1) + bias
    if sh:
        nW = mask.shape[0]
        s = s + mask[torch.arange(s.shape[0]) % nW].unsqueeze(1)
    want = s.logsumexp(-1).reshape(-1)
    assert r.lse.dtype == F64 and r.lse.shape == want.shape
    e = ((r.lse - want).abs().max() / want.abs().max()).item()
    assert e <= 1e-12, f"lse: {e:.3e}"


EXPECT = {   # case: (Bw, R, nW) as the issue's table states them
    "h32": (19, 8, 1), "h48": (13, 5, 1), "h48_long": (42, 5, 1), "h24": (24, 10, 4), "h6": (92, 42, 4),
    "h3": (174, 85, 6), "w9": (24, 10, 4), "w10": (24, 10, 4), "w11": (24, 10, 4),
}


def test_walk_table_walks_unevenly():
    """Every walk case has more windows than workgroups per head and an uneven walk; the shifted ones change the mask
    window along a walk (asserted by walk_shape); h48_long walks 8-9 windows, the others 2-3; h3 changes the mask window
    at every step."""
    assert set(WALKS12) == set(EXPECT)
    assert [big_rows(H, Bw) for H, Bw in ((4, 8), (4, 64), (4, 4096), (48, 4096), (300, 7))] == [8, 64, 64, 5, 1]
    for case, (Bw_, R_, nW_) in EXPECT.items():
        B, Hh, Ww, ws, shift, H, Bw, R = walk_shape(case)
        nW = (Hh // ws) * (Ww // ws)
        assert (Bw, R, nW) == (Bw_, R_, nW_), case
        assert (Bw // R, -(-Bw // R)) == ((8, 9) if case == "h48_long" else (2, 3)), case
        assert (shift > 0) == (nW > 1)
    assert 85 % 6 == 1 and 42 % 4 == 2 and 10 % 4 == 2


@pytest.mark.parametrize("case", list(WALKS12))
def test_walk_bounds_can_see_a_dropped_window(case):
    """The float64 reference alone: dropping any one (window, head) of a walk case moves dbias and the qkv-bias sums by
    at least 4x their bounds."""
    B, Hh, Ww, ws, shift, H, Bw, R = walk_shape(case)
    qkv, do, bias = inputs(B, Hh, Ww, ws, H, 32, 300 + H + ws)
    r = torch_window_attention(qkv, do, bias, B, Hh, Ww, ws, shift, H, 32, F64, images_per_chunk=8)
    drop_b, drop_q = drop_margins(r, H, 32)
    print(f"\n  walk.{case}: one dropped window moves dbias by >= {drop_b:.2e} ({drop_b / FP32_GRADE:.0f}x its bound), "
          f"dqkv_bias by >= {drop_q:.2e} ({drop_q / QKV_BIAS:.1f}x its bound)", end="")
    assert FP32_GRADE * 4 <= drop_b and QKV_BIAS * 4 <= drop_q
