"""vitmi_gemm (gemm.hip, gemm_fast.hip, gemm_fast2.hip, gemm_tile.h, epilogue.h) on every dispatch path against the
float64 reference of tests/gemm_util.py.  Every case starts from vitmi_debug_reset and forces its own path; every operand,
side input and output sits at a leading dimension larger than its row (row + 8 / row + 24) inside a NaN-filled buffer: an
over-read of an input is a gross error, a store outside an output destroys a NaN canary, and an output element that is
not written stays NaN.  The split-K / split-tail workspace is NaN-filled before every call.  Every tile case asks
vitmi_debug_gemm_plan for the plan of its descriptor before the call and fails unless that is the path it is named after
(off_plan).

Paths (gemm_util.PATHS; shapes there):
  generic.bf16 / .fp32  impl = GENERIC: the 64x64 strided kernel, all four layouts
  skinny                AUTO, fp32: gemm_skinny_kernel forms 0 / 1 / 2
  t256.p0-3.persist / .onetile   256x256 tile, main loops 0-3 at one to five k-steps, persistent walk or a tile per workgroup
  t256.walk             320 tiles, row-major and banded tile orders (vitmi_debug_gemm_band -1 / 2 / 5)
  t256.rfold            the fp32 residual streamed through LDS or read by the epilogue (vitmi_debug_gemm_rfold 1 / 0)
  t256.splitk           fp32 plain store with the contraction split over workgroups (17 k-steps: last slice short; 101 k-steps)
  t256.tail             split tail with the finisher kernel or the in-kernel fix-up (needs a 256-CU device)
  t256.padded           VITMI_LAUNCH_ROWS_PADDED: ragged M on the 256x256 tile
  t128                  256x128 tile, whole and ragged shapes and its split-K
  pair, split3          vitmi_gemm_pair (paired and fallen back), ops.gemm_split3
  batch > 1             tests/test_gemm_batched_gpu.py: gemm_small.hip forms 0 / 1 / 2, its split over workgroups, every
                        fallback to the generic kernel and the generic kernel under blockIdx.z

Section 3.1 (test_exact_*): the `integer` family; every product, partial sum and epilogue value is an exact integer (or
half-integer with alpha = 0.5), so C, C2 and colsum_part must be torch.equal to the reference in any summation order.
Section 3.2 (test_accuracy_*): the `normal` and `scaled` families, linear epilogues.  Bounds (largest value measured on an
MI355X in brackets, for information; printed beside the bound with -s):
  * fp32 outputs: rel-to-max (normalised by the row / column scales for `scaled`) <= FP32_GRADE = 2e-6, fp32 sums of exact
    bf16 products; 2e-5 for the K = 12 608 weight gradients (split-K and paired)
    [store 3.7e-7 (skinny form 2, K = 8192), residual 6.8e-7 and patch-pos 7.5e-7 (512 x 768 x 3072), dgelu 6.2e-7 (skinny);
    K = 12 608: split-K 1.4e-7, paired 2.1e-7]
  * bf16 outputs: gemm_util.rounding_check with delta = FP32_GRADE * max |want| — the round-to-nearest-even bf16 of the
    float64 result, the neighbouring value only where the result is within delta of a rounding boundary
    [no element off on any path; the band holds at most 2.72 % of a case's elements (test_gemm_cpu.py asserts <= 3 %)].
    The two 20 M-element shapes (t256.walk, t256.tail) run the `scaled` family only.
  * colsum_part: against float64 sums of the unrounded epilogue values; bound COLSUM = 128 * (2^-24 * max_col sum |v| +
    FP32_GRADE * max |v|) / max |colsum| (an fp32 chain of 128 terms each carrying the fp32-grade error), at most 2e-3
    [3.4e-7 against bounds of 5e-5 ... 1e-4]
Section 3.3 (test_gelu_*): GELU and GELU' at every finite bf16 argument.
  * bf16 tile and generic kernels: rounding_check with delta_gelu = 4 x the worst absolute error of the float32 CPU
    emulation of gemm_tile.h's formulas (gemm_util.tile_gelu_f32) against float64:
      GELU_EMU = 3.26e-7, DGELU_EMU = 2.68e-7  ->  DELTA_GELU = 1.30e-6, DELTA_DGELU = 1.07e-6
    (Abramowitz-Stegun 7.1.26's 1.5e-7 on erfc is the floor; the factor 4 covers the hardware exp2 / rcp and fma contraction)
    and, because an absolute delta says little where gelu(x) ~ x / 2 is tiny, GELU once more over 2^-100 <= |x| <= 1 with
    delta = 4 x GELU_EMU_REL x |x|, the emulation's worst error relative to |x| there:  GELU_EMU_REL = 2.48e-7
    [no element off on any form, depth or store policy]
  * fp32 generic kernel (erff): absolute error <= 4 x that of float32 torch F.gelu / its derivative on the same line where
    torch's result is finite:  GELU_F32 = 8.36e-7, DGELU_F32 = 2.28e-7  ->  3.34e-6, 9.12e-7   [3.8e-7, 1.1e-7]
tests/test_gemm_cpu.py recomputes every figure frozen here and fails if one has drifted.
"""
import ctypes
import functools

import pytest
import torch

import gemm_util as U
from gemm_util import EPI_BIAS_GELU, EPI_DGELU, EPI_PATCH_POS, EPI_RESIDUAL, EPI_STORE, FP32_GRADE, F64

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
LONG_K_GRADE = 2e-5                 # K = 12 608 weight gradients (test_gemm_pair_shares_one_split_k_launch's bound)
COLSUM_CAP = 2e-3
GELU_EMU, DGELU_EMU = 3.26e-7, 2.68e-7
DELTA_GELU, DELTA_DGELU = 4 * GELU_EMU, 4 * DGELU_EMU
GELU_EMU_REL = 2.48e-7
GELU_F32, DGELU_F32 = 8.36e-7, 2.28e-7
HUGE = 64.0                         # |x| >= 64: gelu(x) is x or 0 and gelu'(x) 1 or 0 exactly, in float64 too
LAUNCH_ROWS_PADDED = 2


@pytest.fixture(scope="module")
def ops(lib):
    from vit_torch_amd import ops as _o
    return _o


def variants(path):
    """The switch settings a path is run under: list of dicts."""
    P = U.PATHS.get(path, {})
    if "bands" in P:
        return [dict(band=b) for b in P["bands"]]
    if "rfolds" in P:
        return [dict(rfold=r) for r in P["rfolds"]]
    if "fixups" in P:
        return [dict(fixup=f) for f in P["fixups"]]
    return [dict()]


def force(lib, path, v=None):
    """Every switch to its default, then this path's own."""
    lib.vitmi_debug_reset()
    P, v = U.PATHS.get(path, {}), v or {}
    if path.startswith("t256"):
        lib.vitmi_debug_gemm_tile(1)
    if path == "t128":
        lib.vitmi_debug_gemm_tile(2)
    if "pipe" in P:
        lib.vitmi_debug_gemm_pipe(P["pipe"])
        lib.vitmi_debug_gemm_persist(P["persist"])
    if v.get("band", -1) >= 0:
        lib.vitmi_debug_gemm_band(v["band"])
    if "rfold" in v:
        lib.vitmi_debug_gemm_rfold(v["rfold"])
    if "fixup" in v:
        lib.vitmi_debug_gemm_tail(1)
        lib.vitmi_debug_gemm_tail_fixup(v["fixup"])


def skip_unless_runnable(path):
    if path == "t256.tail" and torch.cuda.get_device_properties(0).multi_processor_count != U.TAIL_CUS:
        pytest.skip("the split-tail shape is laid out for a 256-CU device")


def dev(t, dt=F32):
    return t.to(dt).to("cuda").contiguous()


def gemm(ops, lib, A, B, C, **kw):
    """ops.gemm with the workspace it will use NaN-filled first; returns (takes the tile kernels?, workspace bytes,
    the plan (kind, pipe, deep, splits) the library follows for this call: vitmi_debug_gemm_plan)."""
    d = ops._gemm_desc(A, B, C, **kw)
    need = lib.vitmi_gemm_workspace(ctypes.byref(d))
    if need:
        ws = ops.workspace(need, A.device)
        ws[:ws.numel() // 4 * 4].view(F32).fill_(NAN)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()      # what ops.gemm passes
    fast = bool(lib.vitmi_gemm_uses_fast(ctypes.byref(d)))
    out = [ctypes.c_int(-7) for _ in range(4)]
    assert lib.vitmi_debug_gemm_plan(ctypes.byref(d), *map(ctypes.byref, out)) == 0
    ops.gemm(A, B, C, **kw)
    return fast, need, tuple(o.value for o in out)


def off_plan(path, v, K, epi, c_bf16, plan):
    """Is the plan the path the case is named after?  None, or what is wrong.  (A forced main loop 3 exists only for
    the fp32 residual: everything else resolves to loop 1.  The 256x128 tile splits the fp32 plain store from 16
    64-deep k-steps on: min(256 / tiles, steps / 8) >= 2 slices at the one- and two-tile shapes here.)"""
    kind, pipe, _, splits = plan
    K_, P, v = U.PLAN_KINDS, U.PATHS[path], v or {}
    name = {n: k for k, n in K_.items()}.get(kind, kind)
    if path.startswith("t256") and kind not in (K_["WHOLE"], K_["SPLITK"], K_["TAIL_FINISHER"], K_["TAIL_FIXUP"]):
        return f"plan {name}: not the 256x256 tile"
    if path == "t256.splitk" and not (kind == K_["SPLITK"] and splits > 1):
        return f"plan {name} with {splits} slices: the contraction is not split"
    if path == "t256.tail" and kind != K_["TAIL_FIXUP" if v.get("fixup") else "TAIL_FINISHER"]:
        return f"plan {name}: not the split tail asked for (fixup = {v.get('fixup')})"
    if path == "t128":
        split = epi == EPI_STORE and not c_bf16 and K // 64 >= 16
        if kind != K_["TILE2_SPLITK" if split else "TILE2_WHOLE"] or (splits > 1) != split:
            return f"plan {name} with {splits} slices at K = {K}"
    if "pipe" in P:
        want = P["pipe"] if P["pipe"] < 3 or (epi == EPI_RESIDUAL and not c_bf16) else 1
        if pipe != want:
            return f"main loop {pipe}, not {want}"
    return None


def _inputs(family, M, N, K, in_bf16, side_bf16, big):
    return U.make_inputs(family, M, N, K, None, (M * 31 + N * 17 + K) % 100003 + (7 if family == "scaled" else 0),
                         in_bf16=in_bf16, side_bf16=side_bf16, n_tok=U.NTOK, rows_per_group=U.rpg(M), big_rows=big)


@functools.lru_cache(maxsize=3)
def _product(family, M, N, K, in_bf16, big):
    """a @ b^T in float64 (the operands do not depend on the side inputs' dtype: they are drawn first)."""
    x = _inputs(family, M, N, K, in_bf16, False, big)
    if family == "integer":          # exact in fp32 as well (every partial sum is an integer below 2^24), and much faster
        return (x["a"].float() @ x["b"].float().t()).to(F64)
    return x["a"] @ x["b"].t()


@functools.lru_cache(maxsize=3)
def base(family, M, N, K, in_bf16, side_bf16, big):
    """The inputs of one problem and their float64 product, shared by every epilogue and option set run on it."""
    x = _inputs(family, M, N, K, in_bf16, side_bf16, big)
    x["acc"] = _product(family, M, N, K, in_bf16, big)
    return x


class Run:
    """One vitmi_gemm call on strided, NaN-guarded buffers."""

    def __init__(self, ops, lib, path, x, M, N, K, layout, epi, c_bf16, opts, extras=(8, 24), impl=None):
        from vit_torch_amd._lib import GEMM_AUTO, GEMM_FAST, GEMM_GENERIC
        P = U.PATHS[path]
        akm, bkm = U.LAYOUTS[layout]
        in_dt, cdt = (BF if P["in_bf16"] else F32), (BF if c_bf16 else F32)
        self.M, self.N, self.cdt = M, N, cdt
        self.path, self.K, self.epi, self.c_bf16 = path, K, epi, c_bf16
        self.Mp = Mp = (M + 255) // 256 * 256 if P.get("padded") else M
        e1, e2 = extras
        # (the padding rows of a rows-padded R / AUX hold 0.5: the kernel may read them, and whole tiles of numbers in C's
        # padding are the proof that the 256x256 kernel ran; a column sum that took them in would be off)
        pl = lambda t, e, dt, ra=None, surplus=NAN: U.place(t, e, dt, "cuda", rows_alloc=ra, surplus=surplus)
        _, A = pl(x["a"] if akm else x["a"].t(), e1, in_dt)
        _, B = pl(x["b"] if bkm else x["b"].t(), e2, in_dt)
        nanMN = torch.full((M, N), NAN, dtype=F64)
        self.Cbuf, C = pl(x["C_in"] if "acc" in opts else nanMN, e2, cdt, Mp)
        kw = dict(a_kmajor=akm, b_kmajor=bkm, epilogue=epi,
                  impl={"generic": GEMM_GENERIC, "skinny": GEMM_AUTO, "tile": GEMM_FAST}[P["kind"]] if impl is None else impl)
        if P.get("padded"):
            kw["launch_flags"] = LAUNCH_ROWS_PADDED
        self.C2buf = self.partbuf = self.C2 = self.part = None
        if "bias" in opts:
            kw["bias"] = dev(x["bias"])
        if "alpha" in opts:
            kw["alpha"] = 0.5
        if "acc" in opts:
            kw["accumulate"] = True
        if "C2" in opts:
            self.C2buf, self.C2 = pl(nanMN, e1, in_dt if epi == EPI_RESIDUAL else cdt, Mp)
            kw["C2"] = self.C2
        if "deriv" in opts:
            kw["aux_deriv"] = True
        if epi == EPI_RESIDUAL:
            _, kw["R"] = pl(x["R"], e1, cdt, Mp, 0.5)
            if "gamma" in opts:
                kw["gamma"] = dev(x["gamma"])
            if "rowscale" in opts:
                kw["rowscale"], kw["rows_per_group"] = dev(x["rowscale"]), U.rpg(M)
        elif epi == EPI_DGELU:
            _, kw["aux"] = pl(x["aux"], e1, in_dt, Mp, 0.5)
            if "colsum" in opts:
                G = (M + 127) // 128
                self.partbuf = torch.full((G + 2, N), NAN, device="cuda")
                self.part = kw["colsum_part"] = self.partbuf[:G]
        elif epi == EPI_PATCH_POS:
            kw["pos"], kw["n_tok"] = dev(x["pos"]), U.NTOK
            if "cls" in opts:
                kw["cls"] = dev(x["cls"])
        self.C = C
        self.fast, self.ws, self.plan = gemm(ops, lib, A, B, C, **kw)
        torch.cuda.synchronize()

    def problems(self, P, v=None):
        """Structural failures: the path not taken (under the switch settings v), canaries destroyed, outputs not finite."""
        out = []
        if (P["kind"] == "tile") != self.fast:
            out.append(f"vitmi_gemm_uses_fast = {self.fast}")
        if (P["kind"] == "tile") != (self.plan[0] >= 0):
            out.append(f"vitmi_debug_gemm_plan kind = {self.plan[0]}")
        why = off_plan(self.path, v, self.K, self.epi, self.c_bf16, self.plan) if P["kind"] == "tile" else None
        if why:
            out.append(why)
        if P.get("needs_ws") and not self.ws:
            out.append("no workspace asked for: the contraction was not split")
        for nm, buf, cols in (("C", self.Cbuf, self.N), ("C2", self.C2buf, self.N)):
            if buf is None:
                continue
            if not U.canaries_intact(buf, self.M, cols, rows_alloc=self.Mp):
                out.append(f"{nm}: a store outside the matrix")
            if not torch.isfinite(buf[2:2 + self.M, :cols].float()).all():
                out.append(f"{nm}: non-finite values (an element not written, or an over-read of an input)")
        if P.get("padded") and torch.isnan(self.Cbuf[2 + self.M:2 + self.Mp, :self.N].float()).any():
            out.append("the padding rows were not written: not the 256x256 tile kernel")
        if self.partbuf is not None:
            if not torch.isnan(self.partbuf[self.part.shape[0]:]).all():
                out.append("colsum_part: a row beyond ceil(M / 128) written")
            if not torch.isfinite(self.part).all():
                out.append("colsum_part: non-finite values")
        return out


def check(name, e, bound, failures):
    print(f"\n  {name}: {e:.2e} (bound {bound:.2e})", end="")
    if not e <= bound:
        failures.append(f"{name}: {e:.3e} > {bound:.2e}")


def opt_name(M, N, K, layout, epi, c_bf16, opts, v):
    return (f"{M}x{N}x{K} {layout} {U.EPI_NAMES[epi]} C={'bf16' if c_bf16 else 'fp32'} [{' '.join(opts) or '-'}]"
            + "".join(f" {k}={val}" for k, val in v.items()))


def mismatch(name, got, want64, dt):
    g, w = got.cpu(), want64.to(dt)
    if torch.equal(g, w):
        return None
    bad = (g.double() != w.double()) | torch.isnan(g.double())
    i = bad.nonzero()[0].tolist()
    return f"{name}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: got {g[tuple(i)].item()} want {w[tuple(i)].item()}"


# ----------------------------------------------------------------------------- 3.1 exact index maps ---
PATH_EPIS = [(p, e) for p in U.PATHS for e in U.ALL_EPIS if any(c[4] == e for c in U.cases(p, "3.1"))]


@pytest.mark.parametrize("path,epi", PATH_EPIS, ids=[f"{p}-{U.EPI_NAMES[e]}" for p, e in PATH_EPIS])
def test_exact_on_integers(ops, lib, path, epi):
    """Section 3.1: C, C2 and colsum_part bit-equal to the reference on the `integer` family, every option set, every
    shape of the path, both extras of the leading dimensions in turn."""
    skip_unless_runnable(path)
    P = U.PATHS[path]
    failures, n, kinds = [], 0, set()
    for v in variants(path):
        force(lib, path, v)
        for M, N, K, layout, e, c_bf16, opts in U.cases(path, "3.1"):
            if e != epi or (v != variants(path)[0] and M * N > U.BIG_ELEMS and layout != P["layouts"][0]):
                continue                                  # (a large shape's other variants: the first layout only)
            n += 1
            x = base("integer", M, N, K, P["in_bf16"], c_bf16, U.big_factor(opts, K))
            want = U.reference(None, None, epilogue=epi, acc=x["acc"], **U.ref_kwargs(x, epi, opts))
            name = opt_name(M, N, K, layout, epi, c_bf16, opts, v)
            in_dt = BF if P["in_bf16"] else F32
            checks = [("C", want.C, c_bf16)] if epi != EPI_BIAS_GELU else []      # GELU values: section 3.3
            if want.C2 is not None:
                checks.append(("C2", want.C2, (c_bf16 if epi == EPI_BIAS_GELU else in_dt == BF)))
            for nm, w, b in checks:
                why = U.integer_conditions(w, b)
                assert why is None, f"{name} {nm}: {why}"
            r = Run(ops, lib, path, x, M, N, K, layout, epi, c_bf16, opts, extras=(8, 24) if n % 2 else (24, 8))
            for p_ in r.problems(P, v):
                failures.append(f"{name}: {p_}")
            for nm, w, b in checks:
                got = (r.C if nm == "C" else r.C2)
                m_ = mismatch(f"{name} {nm}", got, w, BF if b else F32)
                if m_:
                    failures.append(m_)
            if "rowscale" in opts:
                drop = (x["rowscale"][torch.arange(M) // U.rpg(M)] == 0)
                if not torch.equal(r.C.cpu()[drop].double(), x["R"][drop]):
                    failures.append(f"{name}: R did not pass through the rows whose rowscale is 0")
            if want.colsum is not None:
                m_ = mismatch(f"{name} colsum_part", r.part, want.colsum, F32)
                if m_:
                    failures.append(m_)
            kinds.add(r.plan[0])
    print(f"\n  {path} {U.EPI_NAMES[epi]}: {n} calls", end="")
    assert n > 0
    if path == "t128" and epi == EPI_STORE:
        assert U.PLAN_KINDS["TILE2_SPLITK"] in kinds and U.PLAN_KINDS["TILE2_WHOLE"] in kinds
    assert not failures, "\n".join(failures[:20]) + (f"\n... {len(failures)} in all" if len(failures) > 20 else "")


def pair_inputs(family, K, M1, N1, seed):
    x0 = base(family, 256, 256, K, True, False, 1.0)
    x1 = U.make_inputs(family, M1, N1, K, None, seed)
    return x0, x1


@pytest.mark.parametrize("second", [(768, 256), (768, 200)], ids=["paired", "unpairable"])
def test_exact_paired_weight_gradients(ops, lib, second):
    """vitmi_gemm_pair on the `integer` family: (256, 256) + (768, 256) over K = 1024 share one split-K launch; with a
    second product of 200 columns (no whole tiles) the call falls back to two launches.  Bit-equal either way."""
    lib.vitmi_debug_reset()
    K = 1024
    M1, N1 = second
    x0, x1 = pair_inputs("integer", K, M1, N1, 77)
    assert ops.gemm_pair_shares_a_launch(256, 256, M1, N1, K) == (N1 % 256 == 0)
    t = []
    for x, (M, N) in ((x0, (256, 256)), (x1, second)):
        _, A = U.place(x["a"].t(), 8, BF, "cuda")
        _, B = U.place(x["b"].t(), 24, BF, "cuda")
        Cbuf, C = U.place(torch.full((M, N), NAN), 24, F32, "cuda")
        t += [A, B, C, Cbuf]
    ops.workspace(1 << 20, "cuda").fill_(0xFF)
    ops.gemm_pair(t[0], t[1], t[2], t[4], t[5], t[6])
    torch.cuda.synchronize()
    for x, C, Cbuf, (M, N) in ((x0, t[2], t[3], (256, 256)), (x1, t[6], t[7], second)):
        want = (x["a"].float() @ x["b"].float().t()).to(F64)
        assert U.integer_conditions(want, False) is None
        assert U.canaries_intact(Cbuf, M, N), "a store outside C"
        assert mismatch(f"pair {M}x{N}", C, want, F32) is None, mismatch(f"pair {M}x{N}", C, want, F32)


@pytest.mark.parametrize("layout", ["nt", "nn"])
def test_exact_bf16x3(ops, lib, layout):
    """ops.gemm_split3 at (300, 96, 160): integers split as hi = x, lo = 0, so the three-part product is exact."""
    lib.vitmi_debug_reset()
    M, N, K = 300, 96, 160
    akm, bkm = U.LAYOUTS[layout]
    x = base("integer", M, N, K, False, False, 1.0)
    _, A = U.place(x["a"] if akm else x["a"].t(), 8, F32, "cuda")
    _, B = U.place(x["b"] if bkm else x["b"].t(), 24, F32, "cuda")
    fails = []
    for opts in (("bias",), ()):
        Cbuf, C = U.place(torch.full((M, N), NAN), 8, F32, "cuda")
        ops.gemm_split3(A, B, C, a_kmajor=akm, b_kmajor=bkm, bias=dev(x["bias"]) if opts else None)
        torch.cuda.synchronize()
        want = U.reference(None, None, acc=x["acc"], **U.ref_kwargs(x, EPI_STORE, opts))
        assert U.integer_conditions(want.C, False) is None
        if not U.canaries_intact(Cbuf, M, N):
            fails.append("a store outside C")
        m_ = mismatch(f"split3 {layout} {opts}", C, want.C, F32)
        if m_:
            fails.append(m_)
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------- 3.2 accuracy against float64 ---
def colsum_bound(v, colsum):
    G, N = colsum.shape
    pad = torch.zeros((G * 128, N), dtype=F64)
    pad[:v.shape[0]] = v.abs()
    s = pad.view(G, 128, N).sum(1).max().item()
    return min(COLSUM_CAP, 128 * (2.0 ** -24 * s + FP32_GRADE * v.abs().max().item()) / colsum.abs().max().item())


def measure(name, got, want64, bf16_out, norm, grade, failures):
    """One output against float64: rel for fp32, rounding_check for bf16; printed beside its bound."""
    g = got.cpu()
    if not bf16_out:
        check(f"{name} rel", U.rel(g, want64, norm), grade, failures)
        return
    wn = want64 / norm
    delta = grade * wn.abs().max().item()
    bad, share, worst = U.rounding_check(g, want64, delta, norm)
    print(f"\n  {name}: {bad} elements off the rounding of float64 (bound 0; band share {share:.2%}, "
          f"worst |err| {worst / wn.abs().max().item():.2e} of max)", end="")
    if bad:
        failures.append(f"{name}: {bad} of {g.numel()} elements are not the bf16 rounding of the float64 result within delta")


ACC_PATHS = [p for p in U.PATHS if any(True for _ in U.cases(p, "3.2"))]


@pytest.mark.parametrize("path", ACC_PATHS)
def test_accuracy_against_float64(ops, lib, path):
    """Section 3.2: `normal` and `scaled` inputs, linear epilogues, richest option set."""
    skip_unless_runnable(path)
    P = U.PATHS[path]
    failures = []
    v = variants(path)[0]
    force(lib, path, v)
    for M, N, K, layout, epi, c_bf16, opts in U.cases(path, "3.2"):
        grade = LONG_K_GRADE if K >= 12608 else FP32_GRADE
        # (the two 20 M-element shapes: `scaled` only, the stricter family; the metric alone takes a second there)
        for family in (("normal", "scaled") if M * N <= U.BIG_ELEMS else ("scaled",)):
            x = base(family, M, N, K, P["in_bf16"], c_bf16, 1.0)
            want = U.reference(None, None, epilogue=epi, acc=x["acc"], **U.ref_kwargs(x, epi, opts))
            name = family + " " + opt_name(M, N, K, layout, epi, c_bf16, opts, v)
            r = Run(ops, lib, path, x, M, N, K, layout, epi, c_bf16, opts)
            for p_ in r.problems(P, v):
                failures.append(f"{name}: {p_}")
            measure(name + " C", r.C, want.C, c_bf16, x["norm"], grade, failures)
            if want.C2 is not None:
                measure(name + " C2", r.C2, want.C2, P["in_bf16"], x["norm"], grade, failures)
            if want.colsum is not None:
                check(name + " colsum_part", U.rel(r.part.cpu(), want.colsum), colsum_bound(want.C, want.colsum), failures)
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("family", ["normal", "scaled"])
def test_accuracy_paired_weight_gradients_at_k_12608(ops, lib, family):
    """(256, 256) + (768, 256) over K = 12 608 tokens in one paired split-K launch, fp32 C: LONG_K_GRADE."""
    lib.vitmi_debug_reset()
    K = 12608
    x0, x1 = pair_inputs(family, K, 768, 256, 78)
    assert ops.gemm_pair_shares_a_launch(256, 256, 768, 256, K)
    t = []
    for x, (M, N) in ((x0, (256, 256)), (x1, (768, 256))):
        _, A = U.place(x["a"].t(), 8, BF, "cuda")
        _, B = U.place(x["b"].t(), 24, BF, "cuda")
        Cbuf, C = U.place(torch.full((M, N), NAN), 24, F32, "cuda")
        t += [A, B, C, Cbuf]
    ops.workspace(1 << 20, "cuda").fill_(0xFF)
    ops.gemm_pair(t[0], t[1], t[2], t[4], t[5], t[6])
    torch.cuda.synchronize()
    failures = []
    for x, C, Cbuf, (M, N) in ((x0, t[2], t[3], (256, 256)), (x1, t[6], t[7], (768, 256))):
        assert U.canaries_intact(Cbuf, M, N), "a store outside C"
        check(f"{family} pair {M}x{N}x{K}", U.rel(C.cpu(), x["a"] @ x["b"].t(), x["norm"]), LONG_K_GRADE, failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------- 3.3 GELU over the whole bf16 line ---
GELU_FORMS = ["t256", "t128", "t256.padded", "generic.bf16", "generic.fp32"]


def gelu_run(ops, lib, form, epi, deriv, depth, policy):
    """The epilogue driven with every finite bf16 value as its argument once: returns (x [M,256] float64 arguments,
    C, C2 or None) on the CPU.  EPI_BIAS_GELU: A one-hot (row m selects k = m mod 256), B the grid: acc = the argument
    exactly.  EPI_DGELU: acc = 1 (A's column 0 and B's row 0 are ones) and AUX the grid."""
    from vit_torch_amd._lib import GEMM_FAST, GEMM_GENERIC
    lib.vitmi_debug_reset()
    tile = form.startswith("t")
    if tile:
        lib.vitmi_debug_gemm_tile(2 if form == "t128" else 1)
        lib.vitmi_debug_gemm_side_depth(depth)
        lib.vitmi_debug_gemm_store_policy(policy)
    padded = form == "t256.padded"
    M, N, K = (264 if padded else 256), 256, 256
    Mp = 512 if padded else M
    dt = F32 if form == "generic.fp32" else BF
    grid = U.gelu_grid()
    arg = grid[torch.arange(M) % 256]                                  # [M, 256]: the argument of output (m, n)
    kw = dict(impl=GEMM_FAST if tile else GEMM_GENERIC, launch_flags=LAUNCH_ROWS_PADDED if padded else 0, aux_deriv=deriv)
    Cbuf, C = U.place(torch.full((M, N), NAN), 8, dt, "cuda", rows_alloc=Mp)
    C2 = None
    if epi == EPI_BIAS_GELU:
        a = torch.zeros((M, K))
        a[torch.arange(M), torch.arange(M) % 256] = 1.0
        _, A = U.place(a, 8, dt, "cuda")
        _, B = U.place(grid.t(), 24, dt, "cuda")
        C2buf, C2 = U.place(torch.full((M, N), NAN), 24, dt, "cuda", rows_alloc=Mp)
        fast, _, _ = gemm(ops, lib, A, B, C, epilogue=epi, C2=C2, **kw)
    else:
        a, b = torch.zeros((M, K)), torch.zeros((K, N))
        a[:, 0], b[0, :] = 1.0, 1.0
        _, A = U.place(a, 8, dt, "cuda")
        _, B = U.place(b, 24, dt, "cuda")
        _, AUX = U.place(arg, 24, dt, "cuda", rows_alloc=Mp, surplus=0.5)
        fast, _, _ = gemm(ops, lib, A, B, C, b_kmajor=False, epilogue=epi, aux=AUX, **kw)
    torch.cuda.synchronize()
    assert fast == tile
    assert U.canaries_intact(Cbuf, M, N, rows_alloc=Mp), "a store outside C"
    return arg.to(F64), C.cpu(), (None if C2 is None else C2.cpu())


def gelu_check(name, x, got, want_fn, huge_pos, huge_neg, bf16_out, delta, failures):
    g = got.double()
    if not torch.isfinite(g).all():
        failures.append(f"{name}: {(~torch.isfinite(g)).sum().item()} non-finite outputs, first at x = {x[~torch.isfinite(g)][0].item()}")
        return
    hp, hn = x >= HUGE, x <= -HUGE
    wp = x[hp] if huge_pos is None else torch.full_like(x[hp], huge_pos)
    if not torch.equal(g[hp], wp):
        failures.append(f"{name}: wrong for huge positive arguments")
    if not torch.equal(g[hn], torch.full_like(g[hn], huge_neg)):
        failures.append(f"{name}: wrong for huge negative arguments")
    want = want_fn(x)
    if bf16_out:
        bad, share, worst = U.rounding_check(got, want, delta)
        print(f"\n  {name}: {bad} elements off the rounding of float64 within delta = {delta:.2e} (bound 0; band share {share:.2%})", end="")
        if bad:
            lo, hi = U.rne_bf16(want - delta), U.rne_bf16(want + delta)
            i = (~((g >= lo) & (g <= hi))).nonzero()[0]
            failures.append(f"{name}: {bad} elements, first at x = {x[tuple(i)].item()}: got {g[tuple(i)].item()} want {want[tuple(i)].item()}")
    else:
        check(f"{name} abs err", (g - want).abs().max().item(), delta, failures)


@pytest.mark.parametrize("form", GELU_FORMS)
def test_gelu_epilogues_over_every_bf16_argument(ops, lib, form):
    """Section 3.3: EPI_BIAS_GELU (C = gelu, C2 = the pre-activation or gelu') and EPI_DGELU without aux_deriv
    (C = 1 * gelu'(AUX)) at every finite bf16 argument; the tile forms with three strips of the side input in flight and
    with one, plain and nt stores."""
    failures = []
    tile = form.startswith("t")
    bf = form != "generic.fp32"
    dg, dd = (DELTA_GELU, DELTA_DGELU) if bf else (4 * GELU_F32, 4 * DGELU_F32)
    for depth, policy in (((3, -1), (1, -1), (3, 2)) if tile else ((3, -1),)):
        tag = f"{form} depth {depth} policy {policy}"
        for deriv in (False, True):
            x, C, C2 = gelu_run(ops, lib, form, EPI_BIAS_GELU, deriv, depth, policy)
            gelu_check(f"{tag} gelu (aux_deriv {int(deriv)})", x, C, U.gelu64, None, 0.0, bf, dg, failures)
            if bf:
                sm = (x.abs() >= U.SMALL_LO) & (x.abs() <= U.SMALL_HI)
                bad, share, _ = U.rounding_check(C[sm], U.gelu64(x[sm]), 4 * GELU_EMU_REL * x[sm].abs())
                print(f"\n  {tag} gelu (aux_deriv {int(deriv)}), |x| <= 1, delta relative to |x|: {bad} elements off (bound 0; band share {share:.2%})", end="")
                if bad:
                    failures.append(f"{tag} gelu (aux_deriv {int(deriv)}): {bad} elements with |x| <= 1 off by more than {4 * GELU_EMU_REL:.1e} |x|")
            if deriv:
                gelu_check(f"{tag} gelu' in C2", x, C2, U.dgelu64, 1.0, 0.0, bf, dd, failures)
            else:
                normal = x.abs() >= 2.0 ** -126                # (the matrix pipe may flush a denormal operand)
                ok = torch.where(normal, C2.double() == x, (C2.double() == x) | (C2.double() == 0))
                if not ok.all():
                    failures.append(f"{tag}: the pre-activation in C2 is not the argument at {int((~ok).sum())} elements")
        x, C, _ = gelu_run(ops, lib, form, EPI_DGELU, False, depth, policy)
        gelu_check(f"{tag} dgelu", x, C, U.dgelu64, 1.0, 0.0, bf, dd, failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------- 3.4 refusals and fall-backs ---
@pytest.mark.parametrize("what", ["A base", "B base", "C base", "lda", "layout tt", "gelu on nn"])
def test_unaligned_or_unbuilt_calls_refuse_the_tile_kernel_and_fall_back(ops, lib, what):
    """impl = GEMM_FAST raises, vitmi_gemm_uses_fast is false, and AUTO gives the exact `integer` result through the
    generic kernel."""
    from vit_torch_amd._lib import GEMM_AUTO, GEMM_FAST, VitmiError
    lib.vitmi_debug_reset()
    M, N, K = 256, 256, 64
    x = base("integer", M, N, K, True, True, 1.0)
    layout, epi, opts = "nt", EPI_STORE, ("bias",)
    if what == "layout tt":
        layout = "tt"
    if what == "gelu on nn":
        layout, epi, opts = "nn", EPI_BIAS_GELU, ("bias", "C2")
    akm, bkm = U.LAYOUTS[layout]

    def off(t, extra, shift):
        """t at leading dimension cols + extra, its base `shift` elements past a 256-byte boundary."""
        rows, cols = t.shape
        flat = torch.full((rows * (cols + extra) + 64,), NAN, dtype=BF, device="cuda")
        v = flat[shift:shift + rows * (cols + extra)].view(rows, cols + extra)[:, :cols]
        v.copy_(t.to(BF))
        return v

    A = off(x["a"] if akm else x["a"].t(), 4 if what == "lda" else 8, 4 if what == "A base" else 0)
    B = off(x["b"] if bkm else x["b"].t(), 8, 4 if what == "B base" else 0)
    mk = lambda: off(torch.full((M, N), NAN), 8, 1 if what == "C base" else 0)
    kw = dict(a_kmajor=akm, b_kmajor=bkm, epilogue=epi, bias=dev(x["bias"]))
    C, C2 = mk(), None
    if "C2" in opts:
        C2 = kw["C2"] = off(torch.full((M, N), NAN), 8, 0)
    d = ops._gemm_desc(A, B, C, impl=GEMM_AUTO, **kw)
    assert not lib.vitmi_gemm_uses_fast(ctypes.byref(d)), "vitmi_gemm_uses_fast must be false"
    with pytest.raises(VitmiError):
        ops.gemm(A, B, C, impl=GEMM_FAST, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(C.float()).all(), "the refused call wrote to C"
    ops.gemm(A, B, C, impl=GEMM_AUTO, **kw)
    torch.cuda.synchronize()
    want = U.reference(None, None, epilogue=epi, acc=x["acc"], **U.ref_kwargs(x, epi, opts))
    if epi == EPI_BIAS_GELU:
        assert torch.isfinite(C.float()).all()
        assert mismatch("C2", C2, want.C2, BF) is None, mismatch("C2", C2, want.C2, BF)
    else:
        assert U.integer_conditions(want.C, True) is None
        assert mismatch("C", C, want.C, BF) is None, mismatch("C", C, want.C, BF)
