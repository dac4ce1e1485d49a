"""CPU checks of tests/elementwise_util.py, the references and inputs of tests/test_elementwise_f64_gpu.py:
  * the conditions the inputs must satisfy: every integer sum and every possible partial sum below 2^24; each colsum case
    on the dispatch form it is listed under; each capped grid past its cap; the cross-entropy inputs tied, separated,
    shifted and scaled as their tests assume;
  * the float32-on-CPU measurements the frozen bounds of the GPU file come from (the constants must not be below them);
  * each reference against an independent formulation.
"""
import math

import torch
import torch.nn.functional as F

import elementwise_util as U
import test_elementwise_f64_gpu as G
from elementwise_util import BF16, F32, F64


# ----------------------------------------------------------------------------- 1. the 2^24 exactness conditions ---
def test_colsum_integer_sums_are_exact_in_fp32():
    for c in U.colsum_cases() + [U.ColsumCase("direct", F32, *U.FOLD_QUEUE_CASE)]:
        x = c.view(c.integers())
        assert x.abs().max() <= 8 and torch.equal(x.to(c.dtype).to(torch.int64), x), c.id      # exact in bf16
        assert x.abs().sum(0).max().item() < U.EXACT_LIMIT, c.id          # the largest possible partial sum
        assert x.sum(0).abs().max().item() < U.EXACT_LIMIT, c.id
        assert x.sum(0).abs().max().item() > 0, c.id


def test_colsum_mul_integer_sums_are_exact_in_fp32():
    for M, N, ldx, ldy in U.COLSUM_MUL_SHAPES:
        xi, yi = U.colsum_mul_integers(M, N, ldx, ldy)
        p = xi[:, :N] * yi[:, :N]
        assert p.abs().max().item() <= 64
        assert p.abs().sum(0).max().item() < U.EXACT_LIMIT and p.sum(0).abs().max().item() < U.EXACT_LIMIT


def test_token_mean_and_relpos_integer_sums_are_exact_in_fp32():
    for B, L, C in U.TOKEN_MEAN_FWD:
        assert 8 * L < U.EXACT_LIMIT and (B * C) % 256 != 0
    for ws, H in U.RELPOS_CASES:
        idx = U.relpos_index(ws)
        most = torch.bincount(idx.reshape(-1)).max().item()
        assert most == ws * ws <= U.RELPOS_LIST          # the centre row: the N diagonal positions; the kernel keeps 256
        assert 8 * most < U.EXACT_LIMIT
    assert any(H > 256 for _, H in U.RELPOS_CASES)        # the head loop's second trip


# ------------------------------------------------------------------------- 2. dispatch forms and capped grids ---
def test_colsum_cases_take_the_forms_they_are_listed_under():
    cases = U.colsum_cases()
    for c in cases:
        assert U.colsum_form(c.dtype, c.M, c.N, c.ld, c.misaligned()) == c.form, c.id
    assert len({c.id for c in cases}) == len(cases)
    have = {(c.form, c.dtype) for c in cases}
    assert have == {("direct", F32)} | {(f, d) for f in ("rows", "vec4", "scalar") for d in (F32, BF16)}
    # the rows kernel's shape edges: 256, 128, 10, 3 (65 of 256 threads idle per row class: 61 idle) and 2 rows per step
    assert [U.rows_per_step(N) for N in (4, 8, 96, 260, 512)] == [256, 128, 10, 3, 2] and 256 % (260 // 4) != 0
    # the partial kernels' row loops take a second trip: 512 splits of 4 rows
    assert all(any(c.form == f and c.dtype == d and c.M > 2048 for c in cases) for f in ("vec4", "scalar") for d in (F32, BF16))
    for c in U.colsum_accuracy_cases():
        assert U.colsum_form(c.dtype, c.M, c.N, c.ld) == c.form
        assert c.M == max(k.M for k in cases if k.form == c.form and k.dtype == c.dtype)


def test_capped_grids_take_a_second_trip():
    blocks = lambda items: (items + 255) // 256
    assert blocks(U.CAST_N // 4 + 1) > 2048 and U.CAST_N % 4 == 3                       # ew_grid: cast, axpy
    B, C, H, p, cls = U.PATCHIFY_CASE
    assert blocks(B * (cls + (H // p) ** 2) * (C * p * p // 4)) > 2048                  # ew_grid: patchify
    M, N, rpg = U.SCALE_CAST_SHAPE
    assert blocks(M * N // 4) > 2048 and M % rpg == 0                                   # ew_grid: scale_cast
    B, Hh, Ww, C = U.PATCH_MERGE_CASES[0]
    assert blocks(B * Hh * Ww * (C // 4)) > 2048                                        # patch_merge
    B, L, C = U.TOKEN_MEAN_BWD
    assert blocks(B * L * C) > 2048                                                     # token_mean_bwd
    M, N = U.GELU_BIG
    assert blocks(M * N // 4) > 4096                                                    # grid_for: gelu_fwd, gelu_bwd
    M, N, ldp, ldd, ldo = U.GELU_SMALL
    assert len({N, ldp, ldd, ldo}) == 4 and min(ldp, ldd, ldo) > N


# ------------------------------------------------------------------------------------- 3. the frozen bounds ---
def test_frozen_bounds_cover_the_float32_measurements():
    m = {"colsum": (U.measure_colsum_f32(), G.F32_COLSUM), "colsum_mul": (U.measure_colsum_mul_f32(), G.F32_COLSUM_MUL),
         "token_mean": (U.measure_token_mean_f32(), G.F32_TOKEN_MEAN),
         "relpos_scatter": (U.measure_relpos_scatter_f32(), G.F32_RELPOS_SCATTER)}
    m.update({"gelu " + k: (v, G.F32_GELU[k]) for k, v in U.measure_gelu_f32().items()})
    m.update({"xent " + k: (v, G.F32_XENT[k]) for k, v in U.measure_xent_f32().items()})
    print("".join(f"\n  {k}: float32 on the CPU {v:.3e}, frozen {f:.2e}" for k, (v, f) in m.items()), end="")
    for k, (v, f) in m.items():
        assert 0 < v <= f <= 1.25 * v, f"{k}: measured {v:.3e}, frozen {f:.2e}"
    assert G.FACTOR == 4.0


# --------------------------------------------------------------------------- 4. independent formulations ---
def test_patch_merge_reference_is_the_oracles_slicing():
    from oracle.swin_ref import PatchMerging
    for B, Hh, Ww, C in U.PATCH_MERGE_CASES:
        pm = PatchMerging((Hh, Ww), C, norm_layer=lambda d: torch.nn.Identity())
        pm.reduction = torch.nn.Identity()
        x = U.normal((B, Hh * Ww, C), Hh + C)
        assert torch.equal(U.patch_merge_ref(x, B, Hh, Ww, C), pm(x))


def test_patchify_reference_is_unfold():
    x = U.normal((2, 3, 32, 32), 1)
    want = F.unfold(x, kernel_size=8, stride=8).transpose(1, 2)
    got = U.patchify_ref(x, 8, 1, 200).view(2, 17, 200)
    assert torch.equal(got[:, 1:, :192], want) and got[:, 0].abs().max() == 0 and got[:, :, 192:].abs().max() == 0
    assert torch.equal(U.patchify_ref(x, 8, 0).view(2, 16, 192), want)


def test_relpos_references():
    for ws, H in [(2, 3), (7, 3), (12, 1)]:
        N, T = ws * ws, (2 * ws - 1) ** 2
        idx = U.relpos_index(ws)
        assert idx.shape == (N, N) and idx.min() == 0 and idx.max() == T - 1
        table = U.normal((T, H), 5).to(F64).requires_grad_(True)
        bias = U.relpos_gather_ref(table, idx)
        for h, i, j in [(0, 0, 0), (H - 1, N - 1, 0), (H - 1, 1, N - 1)]:
            assert bias[h, i, j] == table[idx[i, j], h]
        db = U.ints((H, N, N), 6)
        bias.backward(db.to(F64))                                   # the scatter is the gather's transpose
        assert torch.equal(table.grad, U.relpos_scatter_ref(db, idx, T).to(F64))


def test_cast_reference_rounds_to_nearest_even():
    x = U.cast_input(F32)
    mine, torchs, nan = U.bf16_rne_bits(x), U.bits(x.to(BF16)).to(torch.int32) & 0xFFFF, torch.isnan(x)
    assert torch.equal(mine[~nan], torchs[~nan])
    for b in (mine[nan], torchs[nan]):                              # a NaN stays a NaN, whatever its payload
        assert ((b & 0x7F80) == 0x7F80).all() and ((b & 0x7F) != 0).all()
    for dt in (F32, BF16):
        v = U.cast_input(dt)
        sp = U.cast_specials(dt)
        assert torch.isnan(v).sum() >= 4 and torch.isinf(v).sum() >= 8 and (U.bits(v) == U.bits(sp[1:2])).sum() >= 4   # -0
        assert (v == torch.finfo(dt).max).sum() >= 4
    t = torch.tensor(U._bf16_tie_neighbourhood()[:3] + U._bf16_tie_neighbourhood()[6:9], dtype=F64)
    assert torch.equal(t.to(F32).to(F64), t)                        # the neighbours are fp32 numbers
    assert t.to(F32).to(BF16).to(F64).tolist() == [1.0, 1.0, 1.0078125, 1.0078125, 1.015625, 1.015625]
    assert math.isinf(torch.tensor(torch.finfo(F32).max).to(BF16).item())      # the largest float rounds to infinity


def test_token_mean_and_scale_cast_references():
    xi = U.ints((3, 49, 100), 1)
    assert torch.allclose(U.token_mean_exact(xi).to(F64), xi.to(F64).mean(1), rtol=2.0 ** -23, atol=0)
    dout = U.normal((2, 5), 2)
    r = U.token_mean_bwd_ref(dout, 49, BF16, 2)
    assert r.shape == (2, 49, 5) and torch.equal(r[:, 17], (dout / 49).to(BF16))
    M, N, rpg = U.SCALE_CAST_SHAPE
    for xdt in (F32, BF16):
        x, col, row = U.scale_cast_inputs(xdt)
        assert x.shape == (M, U.SCALE_CAST_LDX) and row.numel() * rpg == M and (row == 0).sum() == 1
        got = U.scale_cast_ref(x[:, :N], col, row, rpg, F32).to(F64)
        m = torch.arange(M)
        want = x[:, :N].to(F64) * col.to(F64) * row.to(F64)[m // rpg][:, None]
        assert ((got - want).abs() <= 2.0 ** -22 * want.abs()).all()              # two roundings
        assert torch.equal(U.scale_cast_ref(x[:, :N], None, None, rpg, BF16), x[:, :N].to(BF16))
    assert U.SCALE_CAST_LDX % 4 == 0 and U.SCALE_CAST_LDO % 4 == 0 and U.SCALE_CAST_LDX != U.SCALE_CAST_LDO


def test_axpy_bound_holds_for_both_roundings():
    x, y = U.axpy_inputs()
    for a in U.AXPY_A:
        want, bound = U.axpy_ref(x, y, a)
        a32 = torch.tensor(a, dtype=F32)
        unfused = y + a32 * x
        fused = want.to(F32)                         # one rounding of the exact value (float64 holds a x + y to 2^-53)
        assert ((unfused.to(F64) - want).abs() <= bound).all() and ((fused.to(F64) - want).abs() <= bound).all()
        assert not ((y + 1.0001 * a32 * x).to(F64) - want).abs().le(bound).all()     # and it is tight enough to notice


def test_gelu_reference_and_inputs():
    for pre, dh in U.gelu_cases():
        p = pre.to(F64).requires_grad_(True)
        y = F.gelu(p)
        y.backward(dh.to(F64))
        wy, wg = U.gelu_ref(pre, dh)
        assert torch.allclose(wy, y.detach(), rtol=1e-13, atol=1e-15) and torch.allclose(wg, p.grad, rtol=1e-13, atol=1e-15)
        assert dh.abs().max() <= 1
        flat, k = pre.reshape(-1), len(U.GELU_POINTS)
        pts = torch.tensor(U.GELU_POINTS, dtype=F32)
        assert torch.equal(U.bits(flat[:k]), U.bits(pts)) and torch.equal(U.bits(flat[-k:]), U.bits(pts))
        body = flat.numel() - 2 * k
        assert flat[k] == -12 and flat[k + body // 2 - 1] == 12 and (flat[k + body // 2:-k].abs() < 12).all()


def test_xent_reference_is_float64_cross_entropy():
    for name, logits, labels in U.xent_accuracy_inputs():
        lg = logits.to(F64).requires_grad_(True)
        rows = F.cross_entropy(lg, labels, reduction="none")
        rows.mean().backward()
        want = U.XentRef(logits, labels)
        assert torch.allclose(want.loss[1:], rows.detach(), rtol=1e-12, atol=1e-12), name
        assert abs(want.loss[0].item() - rows.mean().item()) <= 1e-12 * max(1.0, rows.mean().item()), name
        assert torch.allclose(want.dlogits, lg.grad, rtol=0, atol=1e-15), name
        assert torch.equal(U.first_argmax(logits), logits.argmax(-1)), name       # torch.argmax on the CPU: the first
        assert want.correct[0] == (logits.argmax(-1) == labels).sum() and torch.equal(want.correct[1:].sum(), want.correct[0])


def test_xent_inputs_are_what_their_tests_assume():
    # ties: the maximum sits at exactly the listed indices; the label is the first, a later one, or none of them
    logits, labels, ties = U.xent_tie_inputs()
    kinds = []
    for b, idx in enumerate(ties):
        at = (logits[b] == logits[b].max()).nonzero().reshape(-1).tolist()
        assert at == sorted(idx) and logits[b].max() == U.XENT_TIE_VALUE and idx[-1] < U.XENT_TIE_K
        lab = labels[b].item()
        kinds.append((tuple(i - idx[0] for i in idx), "first" if lab == idx[0] else "later" if lab in idx else "none"))
    assert len(set(kinds)) == len(kinds) == 15
    offs = {k[0] for k in kinds}
    assert {len(o) for o in offs} == {2, 3} and (0, 1) in offs and (0, 64) in offs      # other lanes, the same lane
    assert U.XentRef(logits, labels).correct[1:].tolist() == [int(k[1] == "first") for k in kinds]
    # scale and shift: exact in fp32, the maximum unique and far enough ahead that every other exponential underflows
    base, labels = U.xent_scale_inputs()
    assert torch.equal(base * 256, (base * 256).round()) and base.abs().max() <= 12
    for s in (U.XENT_SHIFT, -U.XENT_SHIFT):
        assert torch.equal((base + s).to(F64), base.to(F64) + s)
    assert torch.equal((base * 1e4).to(F64), base.to(F64) * 1e4)
    for s in U.XENT_SWITCH_SHIFTS:            # rows on both sides of the kernel's switch between its two forms
        assert torch.equal((base + s).to(F64), base.to(F64) + s)
        lse = torch.logsumexp(base.to(F64) + s, -1).abs()
        assert 2 <= (lse < U.XENT_LSE_SWITCH).sum() <= base.shape[0] - 2 and (lse - U.XENT_LSE_SWITCH).abs().min() > 1e-3
    assert (torch.logsumexp(base.to(F64), -1).abs() < U.XENT_LSE_SWITCH).all()
    top = base.topk(2, -1).values
    assert (top[:, 0] - top[:, 1]).min().item() >= U.XENT_UNDERFLOW_GAP
    assert math.exp(-U.XENT_UNDERFLOW_GAP * 1e4) < 2.0 ** -150
    want = U.XentRef(base * 1e4, labels)
    onehot = F.one_hot(base.argmax(-1), base.shape[1]) - F.one_hot(labels, base.shape[1])
    assert (want.dlogits * base.shape[0] - onehot).abs().max() < 1e-45 and torch.isfinite(want.loss).all()
    assert (base.argmax(-1) == labels).sum() not in (0, base.shape[0])
    # -inf: one per row, never at the label;  bad labels: -1 and K, six good rows
    logits, labels, at = U.xent_neginf_inputs()
    assert (at != labels).all() and torch.isinf(logits).sum(1).tolist() == [1] * logits.shape[0]
    want = U.XentRef(logits, labels)
    assert torch.isfinite(want.loss).all() and (want.dlogits[torch.arange(len(at)), at] == 0).all()
    logits, labels, bad = U.xent_bad_label_inputs()
    assert sorted(labels[bad].tolist()) == [-1, logits.shape[1]] and logits.shape[0] == 8
    want = U.XentRef(logits, labels)
    assert torch.isnan(want.loss[[0] + [1 + b for b in bad]]).all() and torch.isnan(want.loss).sum() == 3
    assert want.correct[[1 + b for b in bad]].sum() == 0
    assert torch.allclose(want.dlogits[bad], torch.softmax(logits.to(F64), -1)[bad] / 8, rtol=0, atol=1e-16)
    # the sweeps reach the reduction's second trip and the lanes' second trip
    assert max(B for B, _ in U.xent_sweep_cases()) > 4 * 256 and {63, 64, 65} <= {K for _, K in U.xent_sweep_cases()}
