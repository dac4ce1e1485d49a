"""The conditions tests/test_gemm_batched_gpu.py rests on, checked without a GPU: every case of gemm_batched_util.CASES
lands, by the Python mirror of the dispatch AND by the library's own vitmi_debug_gemm_path (asked with dummy, 16-byte
aligned addresses: nothing is launched, and without a device vitmi_cu_count() is 256, an MI355X's), on the path, form and
workgroups per problem it is named after; the table reaches every condition of gemm_small_form / small_lds_ok from both
sides; no two problems' output windows overlap; and every reference alone meets the conditions of its section
(gemm_util.integer_conditions for the exact one, a rounding band of at most 3 % of the elements for a bf16 accuracy case:
the cap tests/test_gemm_cpu.py asserts.  It is a condition on the inputs, not a measurement of a kernel: a case that
misses it belongs in the exact section only, where K = 1, single products with nothing to average, is)."""
import copy
import ctypes

import pytest
import torch

import gemm_batched_util as BU
import gemm_util as U
from gemm_util import FP32_GRADE

BAND_CAP = 0.03
DUMMY = 1 << 20


def hook_plan(lib, case, g):
    """vitmi_debug_gemm_path for the case's descriptor under the case's switches."""
    lib.vitmi_debug_reset()
    if case.small_hook is not None:
        lib.vitmi_debug_gemm_small(case.small_hook)
    if case.parts_hook:
        lib.vitmi_debug_gemm_small_parts(case.parts_hook)
    d = BU.descriptor(case, g, {s: DUMMY for s in g.sizes}, 1.0)
    out = [ctypes.c_int(-7) for _ in range(3)]
    assert lib.vitmi_debug_gemm_path(ctypes.byref(d), *map(ctypes.byref, out)) == 0
    lib.vitmi_debug_reset()
    return tuple(o.value for o in out)


def test_the_mirror_puts_every_case_on_the_path_its_name_says():
    bad = []
    for name, c in BU.CASES.items():
        g = BU.geometry(c)
        path, form, parts = BU.expected_plan(c, g)
        _, why = BU.small_form(c, g)
        if BU.PATH_NAMES[path] != c.path or (c.path == "small" and form != c.form):
            bad.append(f"{name}: the mirror says {BU.PATH_NAMES[path]} form {form} ({why}), the table {c.path} form {c.form}")
        if c.parts is not None and parts != c.parts:
            bad.append(f"{name}: the mirror says {parts} workgroups per problem, the table {c.parts}")
        if c.path == "generic" and why != c.why:
            bad.append(f"{name}: falls back because of '{why}', not '{c.why}'")
    assert not bad, "\n".join(bad)


def test_the_library_agrees_with_the_mirror_on_every_case(lib):
    bad = []
    for name, c in BU.CASES.items():
        g = BU.geometry(c)
        got, want = hook_plan(lib, c, g), BU.expected_plan(c, g)
        if got != want:
            bad.append(f"{name}: vitmi_debug_gemm_path (path, form, parts) = {got}, the mirror {want}")
    assert not bad, "\n".join(bad)


def test_the_path_query_reports_the_other_paths_too(lib):
    """A 256-aligned bf16 product takes the tile kernels, the classifier head's fp32 product the skinny kernel form 0."""
    from vit_torch_amd._lib import GemmDesc

    def ask(M, N, K, dt):
        d = GemmDesc()
        d.M, d.N, d.K, d.A, d.B, d.C = M, N, K, DUMMY, DUMMY, DUMMY
        d.lda, d.ldb, d.ldc, d.a_kmajor, d.b_kmajor, d.in_dtype, d.c_dtype = K, K, N, 1, 1, dt, dt
        out = [ctypes.c_int(-7) for _ in range(3)]
        assert lib.vitmi_debug_gemm_path(ctypes.byref(d), *map(ctypes.byref, out)) == 0
        return tuple(o.value for o in out)

    lib.vitmi_debug_reset()
    assert ask(512, 768, 768, BU.BF16_CODE) == (BU.PATH_FAST, -1, 0)
    assert ask(256, 10, 768, BU.F32_CODE) == (BU.PATH_SKINNY, 0, 0)
    d = GemmDesc()
    assert lib.vitmi_debug_gemm_path(ctypes.byref(d), None, None, None) == -1            # M = N = K = 0: build_args refuses


STEP_PAST = {"form0 K > 64": dict(K=8), "N > 64": dict(N=8), "K > 256": dict(K=1), "form2 M > 256": dict(M=1), "LDS cap": dict(N=16)}


def test_the_table_reaches_every_condition_from_both_sides():
    """Every condition is failed by a fallback case (first, so it is the one that decides), and every numeric limit has a
    small-kernel case ON it: one step further and the mirror names that limit."""
    failed = {c.why for c in BU.CASES.values() if c.path == "generic"}
    assert failed >= set(BU.CONDITIONS), set(BU.CONDITIONS) - failed
    on = {}
    for name, c in BU.CASES.items():
        for lim in c.at:
            assert c.path == "small"
            past = copy.copy(c)
            for k, step in STEP_PAST[lim].items():
                setattr(past, k, getattr(c, k) + step)
            assert BU.small_form(past, BU.geometry(past)) == (-1, lim), f"{name} does not sit on '{lim}'"
            on.setdefault(lim, []).append(name)
    assert set(on) == set(BU.LIMITS), set(BU.LIMITS) - set(on)
    # both sides of every other condition: each small case passes all of them (the first test), the fallback cases fail them
    assert BU.small_lds(0, 33, 672, 48) <= BU.LDS_CAP < BU.small_lds(0, 33, 673, 48)
    assert BU.CASES["f1.lda_exact"].lda == BU.ru(BU.CASES["f1.lda_exact"].K, 8)
    assert BU.CASES["max_batch.small"].outer * BU.CASES["max_batch.small"].inner == BU.MAX_BATCH


def test_the_parts_cases_stand_on_both_sides_of_eight_row_tiles():
    for f, (_, M, _, _) in BU.PARTS_SHAPES.items():
        assert BU.ru(M, 16) // 16 > 12                       # more than one round of 4 waves x 3 workgroups
        lo, hi = BU.CASES[f"parts.f{f}.tiles7"], BU.CASES[f"parts.f{f}.tiles8"]
        assert (BU.ru(lo.M, 16) // 16, BU.ru(hi.M, 16) // 16) == (7, 8)
        assert lo.outer * lo.inner < 4 * BU.DEVICE_CUS
    for n in ("parts.many_short", "parts.many_tall"):
        c = BU.CASES[n]
        assert BU.geometry(c).batch >= 4 * BU.DEVICE_CUS and c.parts == 1
    assert BU.ru(BU.CASES["parts.many_tall"].M, 16) // 16 >= 8          # only the batch keeps it at one workgroup


def test_no_two_windows_overlap_and_all_lie_inside_their_storage():
    bad = []
    for name, c in BU.CASES.items():
        g = BU.geometry(c)
        used = {s: torch.zeros(n, dtype=torch.int32) for s, n in g.sizes.items()}
        for o in (g.a, g.b, g.c):
            idx = BU.window_index(o, g.outer, g.inner).reshape(-1)
            if idx.min() < BU.FRONT or idx.max() >= g.sizes[o.store] - BU.TAIL:
                bad.append(f"{name}: a window of {o.store} leaves the storage")
                continue
            used[o.store] += torch.bincount(idx, minlength=g.sizes[o.store]).to(torch.int32)
        for s, u in used.items():
            if u.max() > 1:
                bad.append(f"{name}: {int((u > 1).sum())} elements of storage {s} belong to two windows")
        # the 16-byte pieces the small kernel reads along an S-type operand's rows stay inside the row
        if c.path == "small" and c.form in (1, 2) and g.a.ld < BU.ru(g.a.cols, 8):
            bad.append(f"{name}: lda = {g.a.ld} does not cover the last 16-byte piece")
    assert not bad, "\n".join(bad)


def test_every_exact_reference_is_exact():
    bad = []
    for name in BU.exact_cases():
        c = BU.CASES[name]
        why = U.integer_conditions(BU.want(BU.problem(name, "integer"), BU.exact_alpha(name)), c.c_bf16)
        if why:
            bad.append(f"{name}: {why}")
    assert not bad, "\n".join(bad)


def test_the_problems_of_a_batch_differ():
    """Another problem's operands give another integer result: every pair of problems of a small batch differs."""
    for name in ("f0.M16", "f1.K32", "f2.K64", "generic.nt.bf16.cbf16.130"):
        p = BU.problem(name, "integer").prod
        for i in range(p.shape[0]):
            for j in range(i):
                assert not torch.equal(p[i], p[j]), (name, i, j)


@pytest.mark.parametrize("name", [n for n in BU.accuracy_cases() if BU.CASES[n].c_bf16])
def test_rounding_band_of_a_bf16_accuracy_case(name):
    for family in ("normal", "scaled"):
        p = BU.problem(name, family)
        w = BU.want(p, BU.CASES[name].alpha)
        share = U.band_share(w, FP32_GRADE * (w / p.norm).abs().max().item(), p.norm)
        print(f"\n  {name} {family}: band share {share:.2%} (cap {BAND_CAP:.0%})", end="")
        assert share <= BAND_CAP, f"{name} {family}: {share:.2%} of the elements have two admissible roundings"
