"""vitmi_gemm with batch > 1 (gemm_small.hip forms 0 / 1 / 2 and the generic kernel of gemm.hip under blockIdx.z) against
the float64 reference, on the cases of tests/gemm_batched_util.py.  Every case starts from vitmi_debug_reset, sets its own
switches, and asks vitmi_debug_gemm_path for the path, form and workgroups per problem of its descriptor BEFORE the call:
unless they are what the case is named after, it fails without launching (the off_plan rule of test_gemm_gpu.py).  The
operands of a batch lie at two-level batch strides in NaN-filled storages (gemm_batched_util: an S-type operand's pad
columns hold NaN, an output element that is not written stays NaN, a store outside a problem's window destroys a canary).

Groups (gemm_batched_util.CASES; shapes there):
  f0 / f1 / f2   gemm_small_kernel forms 0 (nt) / 1 (nn) / 2 (tn) along K, M and N, the views of ops.th_three_call_fwd / _bwd
                 at (B, T, H, hd) = (2, 197, 3, 48), form 0's scalar store (C off by one element; ldc = N + 2)
  parts          1, 2 and 3 workgroups per problem by vitmi_debug_gemm_small_parts, the heuristic's own choice at 7 and 8
                 row tiles, and batches of 4 x the CU count
  max_batch      65 535 problems on grid.x of the small kernel and on grid.z of the generic one
  fb             one step past every limit of gemm_small_form / small_lds_ok: the generic kernel, by the hook
  generic        impl = GENERIC, all four layouts, bf16 and fp32 operands and outputs, and the long op's shapes

Section 3.1 (test_exact): the `integer` family with alpha 1 or 0.5; every problem of the batch torch.equal to float64.
Section 3.2 (test_accuracy): `normal` and `scaled`, the bounds of test_gemm_gpu.py unchanged (largest value measured on
an MI355X in brackets; printed beside the bound with -s):
  * bf16 outputs: gemm_util.rounding_check, delta = FP32_GRADE * max |want|, zero failing elements
    [no element off on any path; worst |err| 3.8e-3 of max (half a bf16 ulp); the band holds at most 2.91 % of a case's
    elements (f1.K8 scaled), test_gemm_batched_cpu.py asserts <= 3 %]
  * fp32 outputs: rel <= FP32_GRADE = 2e-6   [9.7e-8: bf16 operands (fb.fp32_c); 4.2e-7: fp32 operands (generic.tt, K = 65)]
  plus, for `normal`: the small kernel's result under 2 and 3 workgroups per problem is bit-identical to that under 1 (a
  tile's accumulation order does not depend on the split), and problem z of a batched generic launch is bit-identical to
  the same problem launched alone (blockIdx.z only moves base pointers).
Section 3.3: the six products of talking-heads attention twice, bit-identical; the scores' pad columns never written, the
NaN in the pad columns of S never in an output (the canaries of every case above, restated on the six).
Section 3.4: what build_args refuses of a batched call, with C untouched.

Found by test_exact_on_integers[f1.N8] (161 of 1584 elements, exact zeros where the product was not zero) and fixed in
gemm_small.hip: forms 1 / 2 gave the LDS image of Y a row pitch of N columns but staged, and read, ru16(N); at
N % 16 == 8 the zero piece that pads row k landed on the first 16 bytes of row k + 1 and raced with that row's data.  The
pitch now covers the padded row (y_pitch(Np); small_lds and small_lds_ok follow).  N % 16 == 0, every head dim of the
models, keeps its pitch, LDS size and dispatch."""
import ctypes

import pytest
import torch

import gemm_batched_util as BU
import gemm_util as U
from gemm_util import FP32_GRADE

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def ops(lib):
    from vit_torch_amd import ops as _o
    return _o


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def switches(lib, case, parts_hook=None):
    lib.vitmi_debug_reset()
    if case.small_hook is not None:
        lib.vitmi_debug_gemm_small(case.small_hook)
    ph = case.parts_hook if parts_hook is None else parts_hook
    if ph:
        lib.vitmi_debug_gemm_small_parts(ph)


def ask_path(lib, d):
    out = [ctypes.c_int(-7) for _ in range(3)]
    assert lib.vitmi_debug_gemm_path(ctypes.byref(d), *map(ctypes.byref, out)) == 0
    return tuple(o.value for o in out)


def run(lib, ops, name, family, alpha, parts_hook=None):
    """One batched call of case `name`.  Returns (outputs [batch, M, N] on the CPU, structural failures, problem)."""
    from vit_torch_amd._lib import check
    c = BU.CASES[name]
    g = BU.geometry(c, cus())
    p = BU.problem(name, family, cus())
    a, b = BU.stored(p, g)
    st, idx = BU.build_storages(g, a, b, BF if c.in_bf16 else F32, BF if c.c_bf16 else F32, "cuda")
    d = BU.descriptor(c, g, {s: t.data_ptr() for s, t in st.items()}, alpha)
    switches(lib, c, parts_hook)
    # the path the case is named after, or no launch
    want = BU.expected_plan(c, g, cus())
    if parts_hook:
        want = (want[0], want[1], parts_hook)
    got = ask_path(lib, d)
    assert got == want, f"{name}: vitmi_debug_gemm_path (path, form, parts) = {got}, the case is named after {want}"
    assert BU.PATH_NAMES[got[0]] == c.path and (c.path != "small" or got[1] == c.form), f"{name}: {got}"
    assert c.parts is None or parts_hook or got[2] == c.parts, f"{name}: {got[2]} workgroups per problem, not {c.parts}"
    check(lib.vitmi_gemm(ctypes.byref(d), ops._stream()), "vitmi_gemm(batched)")
    torch.cuda.synchronize()
    out, clean = BU.read_windows(st[g.c.store].cpu(), idx)
    bad = []
    if not clean:
        bad.append(f"{name}: a store outside the problems' M x N windows")
    if not torch.isfinite(out.float()).all():
        n = int((~torch.isfinite(out.float())).sum())
        bad.append(f"{name}: {n} non-finite outputs (an element not written, or a pad column / another storage's NaN read)")
    return out, bad, p


def mismatch(name, got, want64, dt):
    """None, or how the batch differs from the reference (per problem)."""
    w = want64.to(dt)
    if torch.equal(got, w):
        return None
    bad = (got.double() != w.double()) | torch.isnan(got.double())
    i = bad.nonzero()[0].tolist()
    probs = bad.flatten(1).any(1).nonzero().flatten().tolist()
    return (f"{name}: {int(bad.sum())} of {bad.numel()} elements differ, in problems {probs[:8]}{'...' if len(probs) > 8 else ''}; "
            f"first at (z, m, n) = {i}: got {got[tuple(i)].item()} want {w[tuple(i)].item()}")


# ------------------------------------------------------------------------------------ 3.1 exact ---
@pytest.mark.parametrize("name", BU.exact_cases())
def test_exact_on_integers(lib, ops, name):
    """Section 3.1: every problem of the batch bit-equal to the float64 reference on the `integer` family."""
    c = BU.CASES[name]
    alpha = BU.exact_alpha(name)
    got, bad, p = run(lib, ops, name, "integer", alpha)
    want = BU.want(p, alpha)
    why = U.integer_conditions(want, c.c_bf16)
    assert why is None, f"{name}: a broken case: {why}"
    m = mismatch(name, got, want, BF if c.c_bf16 else F32)
    n_bad = int((~(got.double() == want)).sum())
    print(f"\n  {name} alpha {alpha}: {got.shape[0]} problems, {n_bad} elements differ (bound 0)", end="")
    if m:
        bad.append(m)
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------------- 3.2 accuracy ---
def measure(tag, got, want64, bf16_out, norm, failures):
    """The whole batch against float64: rel for fp32, rounding_check for bf16; printed beside its bound."""
    if not bf16_out:
        e = U.rel(got, want64, norm)
        print(f"\n  {tag} rel: {e:.2e} (bound {FP32_GRADE:.2e})", end="")
        if not e <= FP32_GRADE:
            failures.append(f"{tag} rel: {e:.3e} > {FP32_GRADE:.2e}")
        return
    top = (want64 / norm).abs().max().item()
    n_bad, share, worst = U.rounding_check(got, want64, FP32_GRADE * top, norm)
    print(f"\n  {tag}: {n_bad} elements off the rounding of float64 (bound 0; band share {share:.2%}, "
          f"worst |err| {worst / top:.2e} of max)", end="")
    if n_bad:
        failures.append(f"{tag}: {n_bad} of {got.numel()} elements are not the bf16 rounding of the float64 result within delta")


def alone(lib, ops, name, family, alpha, z):
    """Problem z of the case as a call of its own: batch = 1, impl = GENERIC, the operands copied out of the batch."""
    from vit_torch_amd._lib import GEMM_GENERIC
    c = BU.CASES[name]
    g = BU.geometry(c, cus())
    a, b = BU.stored(BU.problem(name, family, cus()), g)
    in_dt, c_dt = (BF if c.in_bf16 else F32), (BF if c.c_bf16 else F32)
    _, A = U.place(a[z], 8, in_dt, "cuda")
    _, B = U.place(b[z], 24, in_dt, "cuda")
    Cbuf, C = U.place(torch.full((c.M, c.N), NAN), 8, c_dt, "cuda")
    lib.vitmi_debug_reset()
    ops.gemm(A, B, C, a_kmajor=g.akm, b_kmajor=g.bkm, alpha=alpha, impl=GEMM_GENERIC)
    torch.cuda.synchronize()
    assert U.canaries_intact(Cbuf, c.M, c.N)
    return C.cpu()


@pytest.mark.parametrize("name", BU.accuracy_cases())
def test_accuracy_against_float64(lib, ops, name):
    """Section 3.2: `normal` and `scaled` against float64 with alpha applied in float64; the bit-identity of the split
    (small kernel) and of a problem launched alone (generic group) on `normal`."""
    c = BU.CASES[name]
    failures = []
    for family in ("normal", "scaled"):
        got, bad, p = run(lib, ops, name, family, c.alpha)
        failures += bad
        measure(f"{name} {family}", got, BU.want(p, c.alpha), c.c_bf16, p.norm, failures)
        if family != "normal":
            continue
        if c.group == "parts" and c.parts_hook == 1:
            for parts in (2, 3):
                other, bad, _ = run(lib, ops, name, family, c.alpha, parts_hook=parts)
                failures += bad
                n = int((other.view(torch.int16) != got.view(torch.int16)).sum())
                print(f"\n  {name} {family}: {n} elements differ between {parts} and 1 workgroups per problem (bound 0)", end="")
                if n:
                    failures.append(f"{name}: {n} elements differ between {parts} and 1 workgroups per problem")
        if c.group == "generic":
            n = 0
            for z in range(got.shape[0]):
                one = alone(lib, ops, name, family, c.alpha, z)
                n += int((one.view(torch.int32 if one.dtype == F32 else torch.int16)
                          != got[z].view(torch.int32 if one.dtype == F32 else torch.int16)).sum())
            print(f"\n  {name} {family}: {n} elements differ between the batched launch and each problem alone (bound 0)", end="")
            if n:
                failures.append(f"{name}: {n} elements differ between the batched launch and the problems launched alone")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------- 3.3 determinism and the pad contract ---
def test_the_six_products_twice_are_bit_identical_and_keep_the_pad_contract(lib, ops):
    """q k^T, P' v, dO v^T, dS k, P'^T dO, dS^T q at (B, T, H, hd) = (2, 197, 3, 48) on the views the three-call form uses,
    twice: the same bits; nothing outside the outputs' windows written (the scores' pad columns 197 .. 200 among it); no
    NaN of the pad columns of S / P' / dS in an output."""
    failures = []
    for name in BU.SIX_PRODUCTS:
        c = BU.CASES[name]
        g = BU.geometry(c)
        assert (g.outer, c.M, g.inner) == (BU.TH[0], BU.TH[1], BU.TH[2])
        if c.form == 0:                                    # the pad columns exist, and they are outside every window
            assert g.c.ld == BU.ru(c.N, 8) > c.N
        else:                                              # S is read at its padded pitch, the pad columns NaN
            assert g.a.ld == BU.ru(g.a.cols, 8) > g.a.cols
        first, bad, _ = run(lib, ops, name, "normal", c.alpha)
        failures += bad
        second, bad, _ = run(lib, ops, name, "normal", c.alpha)
        failures += bad
        n = int((first.view(torch.int16) != second.view(torch.int16)).sum())
        print(f"\n  {name}: {n} elements differ between two runs (bound 0)", end="")
        if n:
            failures.append(f"{name}: {n} elements differ between two runs")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------- 3.4 refusals ---
EPI_BIAS_GELU, EPI_RESIDUAL = U.EPI_BIAS_GELU, U.EPI_RESIDUAL
REFUSALS = {
    "epilogue gelu": dict(epilogue=EPI_BIAS_GELU),
    "epilogue residual": dict(epilogue=EPI_RESIDUAL),
    "accumulate": dict(accumulate=1),
    "batch % batch_inner": dict(batch_inner=4),
    "batch 65536": dict(batch=65536, batch_inner=1),
}


@pytest.mark.parametrize("what", REFUSALS)
def test_out_of_contract_batched_calls_are_refused_before_any_launch(lib, ops, what):
    """VITMI_E_BADARG (-1), for the path query too, and a NaN-filled C untouched.  (The descriptor of a batch of 6; for
    65 536 only the count changes: the call is refused before anything is read.)"""
    for fp32_c in (False, True):                           # (accumulate alone is legal only with an fp32 C)
        c = BU.CASES["fb.fp32_c" if fp32_c else "f0.M16"]
        g = BU.geometry(c)
        a, b = BU.stored(BU.problem(c.name, "integer"), g)
        st, idx = BU.build_storages(g, a, b, BF, F32 if fp32_c else BF, "cuda")
        d = BU.descriptor(c, g, {s: t.data_ptr() for s, t in st.items()}, 1.0)
        if REFUSALS[what].get("epilogue") == EPI_RESIDUAL:
            d.R, d.ldr, d.r_dtype = d.C, d.ldc, d.c_dtype
        for k, v in REFUSALS[what].items():
            setattr(d, k, v)
        lib.vitmi_debug_reset()
        out = [ctypes.c_int(-7) for _ in range(3)]
        assert lib.vitmi_debug_gemm_path(ctypes.byref(d), *map(ctypes.byref, out)) == -1
        rc = lib.vitmi_gemm(ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()
        print(f"\n  {what}, C {'fp32' if fp32_c else 'bf16'}: rc = {rc} (expected -1): {lib.vitmi_last_error_string().decode()}", end="")
        assert rc == -1
        assert torch.isnan(st[g.c.store].float()).all(), "the refused call wrote to C"
