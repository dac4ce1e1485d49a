"""Host-side half of the LayerNorm tests: the float64 closed form against autograd, the fp32 emulation of the kernels
against half of every frozen bound on every input tests/test_layernorm_gpu.py runs, and proof that the case tables reach
the kernel forms, row loops and block counts they claim (tests/ln_util.py restates the dispatcher of csrc/layernorm.hip;
the library's own workspace query is the cross-check)."""
import pytest
import torch
import torch.nn.functional as F

import ln_util as U


def test_closed_form_backward_equals_float64_autograd():
    g = torch.Generator("cpu").manual_seed(7)
    for M, D, eps in ((5, 12, 1e-6), (19, 96, 1e-5), (4, 2048, 1e-6)):
        x = (2 * torch.randn(M, D, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
        gamma = (1 + 0.1 * torch.randn(D, generator=g, dtype=torch.float64)).requires_grad_(True)
        beta = (0.1 * torch.randn(D, generator=g, dtype=torch.float64)).requires_grad_(True)
        dy, gin = torch.randn(M, D, generator=g, dtype=torch.float64), torch.randn(M, D, generator=g, dtype=torch.float64)
        y = F.layer_norm(x, (D,), gamma, beta, eps=U.f32(eps))
        y.backward(dy)
        wy, mean, rstd = U.ref_fwd(x.detach(), gamma.detach(), beta.detach(), eps)
        r = U.ref_bwd(dy, x.detach(), mean, rstd, gamma.detach(), gin)

        def rel(a, b):
            return ((a - b).abs().max() / b.abs().max()).item()
        assert rel(wy, y.detach()) <= 1e-12
        assert rel(r.g_out, gin + x.grad) <= 1e-12
        assert rel(r.dgamma, gamma.grad) <= 1e-12 and rel(r.dbeta, beta.grad) <= 1e-12
        assert rel(r.gsum, (gin + x.grad).sum(0)) <= 1e-12 and torch.equal(r.gb, r.g_out)
        col, row = torch.randn(D, generator=g, dtype=torch.float64), torch.tensor([0.0, 1.25, 2.0])
        rpg = -(-M // 3)
        r = U.ref_bwd(dy, x.detach(), mean, rstd, gamma.detach(), gin, col, row, rpg)
        want = (gin + x.grad) * col * row[torch.arange(M) // rpg][:, None]
        assert rel(r.gb, want) <= 1e-12 and rel(r.gsum, want.sum(0)) <= 1e-12 and rel(r.g_out, gin + x.grad) <= 1e-12


def test_bounds_are_complete_and_positive():
    assert set(U.BOUNDS) == {(c, d) for c in U.CLASSES_FWD + U.CLASSES_BWD for d in U.DATA}
    assert all(0 < b < 1e-4 for b in U.BOUNDS.values())


@pytest.mark.parametrize("c", U.ALL_FWD, ids=U.ids(U.ALL_FWD))
def test_fwd_emulation_within_half_of_each_bound(c):
    for k, e in U.fwd_emu_errors(c, U.fwd_inputs(c)).items():
        assert e <= 0.5 * U.BOUNDS[(k, c.data)], f"{c.id}: emulated {k} error {e:.3e} > half of {U.BOUNDS[(k, c.data)]:.3e}"


@pytest.mark.parametrize("c", U.ALL_BWD, ids=U.ids(U.ALL_BWD))
def test_bwd_emulation_within_half_of_each_bound(c):
    for k, e in U.bwd_emu_errors(c, U.bwd_inputs(c)).items():
        assert e <= 0.5 * U.BOUNDS[(k, c.data)], f"{c.id}: emulated {k} error {e:.3e} > half of {U.BOUNDS[(k, c.data)]:.3e}"


@pytest.mark.parametrize("c", U.ROUND_TRIP, ids=U.ids(U.ROUND_TRIP))
def test_round_trip_emulation_within_half_of_the_summed_bounds(c):
    extra = U.BOUNDS[("mean", c.data)] + U.BOUNDS[("rstd", c.data)]
    for k, e in U.round_trip_emu_errors(c, U.bwd_inputs(c)).items():
        assert e <= 0.5 * (U.BOUNDS[(k, c.data)] + extra), f"{c.id}: emulated round-trip {k} error {e:.3e}"


def test_bf16_rule_accepts_the_rounded_emulation_and_no_more():
    """A bf16 store of a value within the fp32 bound passes the bf16 rule (2^-8 |want|, bf16's unit roundoff: with 2^-9 the
    correctly rounded store itself fails); the same value one bf16 step off does not."""
    c = next(c for c in U.FWD_FORMS if c.ydt == "bf16" and c.D == 768)
    inp = U.fwd_inputs(c)
    y, _, _ = U.emu_fwd(inp["x"], inp["gamma"], inp["beta"], c.eps, c.form)
    wy, _, _ = U.ref_fwd(inp["x"], inp["gamma"], inp["beta"], c.eps)
    sy, _ = U.fwd_scales(inp["x"], inp["beta"])
    yb = y.to(torch.bfloat16)
    assert U.norm_err(yb, wy, sy, True) <= U.BOUNDS[("y", c.data)]
    half = ((yb.double() - wy).abs() - 2.0 ** -9 * wy.abs()) / sy
    assert half.max() > U.BOUNDS[("y", c.data)]                 # what a 2^-9 rule would have made of correct rounding
    off = (yb.float() * (1 + 2.0 ** -6)).to(torch.bfloat16)     # one or two bf16 steps away from zero
    assert (off != yb).all() and U.norm_err(off, wy, sy, True) > U.BOUNDS[("y", c.data)]


def test_ids_are_unique():
    for cases in (U.ALL_FWD, U.ALL_BWD):
        assert len(set(U.ids(cases))) == len(cases)


# --------------------------------------------------------------------------- the tables reach what they claim ---
def _forms_hit(cases):
    return {c.form for c in cases}


def test_every_form_is_hit_in_both_directions():
    want8 = {(8,) + f for f in U.FORMS8}
    want4 = {(4, 64, nv) for nv in U.NVS4}
    for name, cases in (("fwd", U.ALL_FWD), ("bwd", U.ALL_BWD)):
        hit = _forms_hit(cases)
        assert want8 <= hit, f"{name}: 8-element forms never launched: {sorted(want8 - hit)}"
        assert want4 <= hit, f"{name}: 4-element NV variants never launched: {sorted(want4 - hit)}"
    # the three ways into the 4-element kernels
    for cases in (U.FWD_FOUR, U.BWD_FOUR):
        assert all(c.form[0] == 4 for c in cases)
        assert {c.D for c in cases if c.D % 8 == 4} >= {4, 12, 100, 516, 772, 1028, 2044}
        assert any(c.D == 768 and not c.force4 and c.xs % 8 == 4 for c in cases)
        assert {c.D for c in cases if c.force4} == {96, 768, 2048}
    assert {c.D for c in U.FWD_FORMS} == {c.D for c in U.BWD_FORMS} == set(U.FORM_D + U.EDGE_D)
    assert all(c.form[0] == 8 for c in U.FWD_FORMS + U.BWD_FORMS)
    # the full dtype product at one D per form
    for D in U.FORM_D:
        assert {(c.xdt, c.ydt) for c in U.FWD_FORMS if c.D == D} == set(U.FWD_DTYPES)
        assert {(c.dy, c.r, c.gb) for c in U.BWD_FORMS if c.D == D and c.gb} | \
               {(c.dy, c.r, c.dy) for c in U.BWD_FORMS if c.D == D and not c.gb} == set(U.BWD_DTYPES)
    for flag in ("g_in", "gsum"):
        assert {getattr(c, flag) for c in U.BWD_FORMS} == {True, False}
    assert {bool(c.gb) for c in U.BWD_FORMS} == {True, False}
    # partially live last row group for LPR 16 and 32
    assert all(c.M % U.rpw_of(c.form) for c in U.FWD_FORMS + U.BWD_FORMS if U.rpw_of(c.form) > 1)
    assert {c.eps for c in U.ALL_BWD} == {c.eps for c in U.ALL_FWD} == {1e-6, 1e-5}


def test_every_loop_case_loops():
    hit = {"fwd": set(), "bwd": set()}
    for name, cases, blocks in (("fwd", U.FWD_LOOPS, U.fwd_blocks), ("bwd", U.BWD_LOOPS, U.bwd_blocks)):
        for c in cases:
            nb = blocks(c.M, c.form)
            lo, hi = U.groups_per_wave(c.M, c.form, nb)
            groups = -(-c.M // U.rpw_of(c.form))
            assert lo >= 3 and hi > lo and groups % (nb * 4) != 0, f"{c.id}: waves walk {lo}..{hi} row groups"
            assert c.M * c.D * 4 <= 210e6
            hit[name].add(c.form)
    assert hit["fwd"] == {(8, 16, 1), (8, 32, 3), (8, 64, 4)}
    assert hit["bwd"] == {(8,) + f for f in U.FORMS8} | {(4, 64, nv) for nv in U.NVS4}
    for c in U.DETERMINISM:
        assert c in U.BWD_LOOPS


def test_block_counts_match_the_library(lib):
    """vitmi_layernorm_bwd_workspace(M, D) == blocks * 3 * D * 4 with the restated block counts (a host-only query)."""
    shapes = {(c.M, c.D) for c in U.ALL_BWD} | {(50432, 768), (1, 4), (4097, 2048), (3073, 1028)}
    for M, D in sorted(shapes):
        assert lib.vitmi_layernorm_bwd_workspace(M, D) == U.workspace_blocks(M, D) * 3 * D * 4, (M, D)
    for c in U.ALL_BWD:                                  # the form a case takes never needs more than is reserved
        assert U.bwd_blocks(c.M, c.form) <= U.workspace_blocks(c.M, c.D)
