"""What the tile GEMM would launch (plan_fast, gemm_fast.hip) on the training step's own shapes, asked through
vitmi_gemm_workspace / vitmi_gemm_pair_workspace / vitmi_debug_gemm_plan.  Nothing is launched: the descriptors carry
dummy, 16-byte-aligned addresses, and without a device vitmi_cu_count() is 256, an MI355X's.

Expected values, from the rules (BK = 64 for both tile sizes' k-steps; ViT-B/16, 256 images: M = 50 432 tokens):
  split-K, 256x256: up to 128 tiles and >= 16 k-steps: s = min(256 / tiles, steps / 8); ksps = ceil(steps / s);
                    splits = ceil(steps / ksps); workspace = splits * M * N * 4
  split tail:       tiles > 256 CUs, remainder r with 3 r <= 256, >= 36 k-steps (>= 6 when forced): 3 slices,
                    workspace = 3 * M * N * 4 + 4096
  split-K, 256x128: up to 256 tiles, the same formula
The workspace tests also pass on a build without the plan query (VITMI_LIB), where they pin the same numbers."""
import ctypes

import pytest

from gemm_util import PLAN_KINDS as K_

BF16, F32 = 1, 0
EPI_STORE, EPI_RESIDUAL = 0, 2
TOK, D = 256 * 197, 768
WS_PTR = 1 << 20                    # a dummy, aligned workspace address


def desc(M, N, K, layout, *, c=BF16, epi=EPI_STORE, **k):
    from vit_torch_amd._lib import GemmDesc
    akm, bkm = {"nt": (1, 1), "nn": (1, 0), "tn": (0, 0)}[layout]
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.A = d.B = d.C = 256
    d.lda, d.ldb, d.ldc = (K if akm else M), (K if bkm else N), N
    d.a_kmajor, d.b_kmajor = akm, bkm
    d.in_dtype, d.c_dtype, d.epilogue = BF16, c, epi
    if epi == EPI_RESIDUAL:
        d.R, d.ldr, d.r_dtype = 256, N, c
    for name, v in k.items():
        setattr(d, name, v)
    return d


def plan(lib, d, ws_bytes=None, ws_ptr=WS_PTR):
    """(kind, pipe, deep, splits) with a workspace of `ws_bytes` (default: what vitmi_gemm_workspace asks for)."""
    need = lib.vitmi_gemm_workspace(ctypes.byref(d))
    ws_bytes = need if ws_bytes is None else ws_bytes
    d.workspace, d.workspace_bytes = (ws_ptr if ws_bytes else None), ws_bytes
    out = [ctypes.c_int(-7) for _ in range(4)]
    assert lib.vitmi_debug_gemm_plan(ctypes.byref(d), *map(ctypes.byref, out)) == 0
    d.workspace, d.workspace_bytes = None, 0
    return tuple(o.value for o in out)


proj_wgrad = lambda: desc(D, D, TOK, "tn", c=F32)
qkv_wgrad = lambda: desc(3 * D, D, TOK, "tn", c=F32)
fc2_fwd = lambda: desc(TOK, D, 4 * D, "nt", c=F32, epi=EPI_RESIDUAL)
proj_fwd = lambda: desc(TOK, D, D, "nt", c=F32, epi=EPI_RESIDUAL)
swin_wgrad = lambda: desc(96, 96, 401408, "tn", c=F32)
TAIL_WS = 3 * TOK * D * 4 + 4096

# name: (descriptor, switches (hook, value), kind, splits, workspace bytes)
TABLE = {
    "proj wgrad": (proj_wgrad, (), "SPLITK", 28, 28 * D * D * 4),                    # 9 tiles, 788 steps: 28 slices of 29
    "qkv wgrad": (qkv_wgrad, (), "SPLITK", 9, 9 * 3 * D * D * 4),                     # 27 tiles: 9 slices of 88
    "fc2 forward": (fc2_fwd, (), "TAIL_FINISHER", 3, TAIL_WS),                        # 591 tiles, remainder 79, 48 steps
    "fc2 forward, tail off": (fc2_fwd, (("tail", 0),), "WHOLE", 1, 0),
    "proj forward": (proj_fwd, (), "WHOLE", 1, 0),                                    # 12 steps < 36
    "proj forward, tail forced": (proj_fwd, (("tail", 1),), "TAIL_FINISHER", 3, TAIL_WS),
    "proj forward, tail forced, fix-up": (proj_fwd, (("tail", 1), ("tail_fixup", 1)), "TAIL_FIXUP", 3, TAIL_WS),
    # one 256x128 tile, 401 408 / 64 = 6 272 steps: s = min(256, 784) = 256, ksps = ceil(6272 / 256) = 25, splits = ceil(6272 / 25)
    "swin stage-0 wgrad": (swin_wgrad, (), "TILE2_SPLITK", 251, 251 * 96 * 96 * 4),
}


def switch(lib, switches):
    lib.vitmi_debug_reset()
    for hook, v in switches:
        getattr(lib, "vitmi_debug_gemm_" + hook)(v)


def test_the_step_shapes_values():
    assert 28 * D * D * 4 == 66_060_288 and 9 * 3 * D * D * 4 == 63_700_992 and TAIL_WS == 464_785_408
    assert 251 * 96 * 96 * 4 == 9_252_864


@pytest.mark.parametrize("case", TABLE)
def test_workspace_of_the_step_shapes(lib, case):
    mk, switches, _, _, ws = TABLE[case]
    switch(lib, switches)
    assert lib.vitmi_gemm_workspace(ctypes.byref(mk())) == ws


def test_workspace_of_the_paired_weight_gradients(lib):
    """36 tiles: 7 slices of 113 steps."""
    lib.vitmi_debug_reset()
    assert lib.vitmi_gemm_pair_workspace(ctypes.byref(qkv_wgrad()), ctypes.byref(proj_wgrad())) == 7 * (3 * D * D + D * D) * 4 == 66_060_288


@pytest.mark.parametrize("case", TABLE)
def test_plan_of_the_step_shapes(lib, case):
    mk, switches, kind, splits, _ = TABLE[case]
    switch(lib, switches)
    got = plan(lib, mk())
    assert (got[0], got[3]) == (K_[kind], splits), got


def test_a_workspace_one_byte_short_falls_to_the_next_choice(lib):
    lib.vitmi_debug_reset()
    for mk, full in ((proj_wgrad, "SPLITK"), (fc2_fwd, "TAIL_FINISHER")):
        need = lib.vitmi_gemm_workspace(ctypes.byref(mk()))
        assert plan(lib, mk(), need)[0] == K_[full]
        assert plan(lib, mk(), need - 1)[0] == K_["WHOLE"]
        assert plan(lib, mk(), 0)[0] == K_["WHOLE"]
    need = lib.vitmi_gemm_workspace(ctypes.byref(swin_wgrad()))
    assert plan(lib, swin_wgrad(), need - 1)[0] == K_["TILE2_WHOLE"]


def test_a_misaligned_workspace_is_treated_as_absent(lib):
    lib.vitmi_debug_reset()
    need = lib.vitmi_gemm_workspace(ctypes.byref(proj_wgrad()))
    assert plan(lib, proj_wgrad(), need + 64, ws_ptr=WS_PTR + 16)[0] == K_["SPLITK"]
    assert plan(lib, proj_wgrad(), need + 64, ws_ptr=WS_PTR + 4)[0] == K_["WHOLE"]


def test_main_loop_of_each_layout(lib):
    pipe = lambda d: plan(lib, d)[1]
    lib.vitmi_debug_reset()
    assert pipe(desc(TOK, 3 * D, D, "nt")) == 2                        # qkv forward
    assert pipe(desc(TOK, D, 3 * D, "nn")) == 1                        # qkv data gradient
    assert pipe(qkv_wgrad()) == 1                                      # tn
    # the fp32 residual streams R through LDS at K >= 640, unless something scales the branch or R is bf16
    assert pipe(proj_fwd()) == 3 and pipe(fc2_fwd()) == 3
    assert pipe(desc(TOK, D, 576, "nt", c=F32, epi=EPI_RESIDUAL)) == 2
    assert pipe(desc(TOK, D, D, "nt", c=F32, epi=EPI_RESIDUAL, gamma=256)) == 2
    assert pipe(desc(TOK, D, D, "nt", c=F32, epi=EPI_RESIDUAL, rowscale=256, rows_per_group=197)) == 2
    assert pipe(desc(TOK, D, D, "nt", c=F32, epi=EPI_RESIDUAL, C2=256, ldc2=D)) == 2
    assert pipe(desc(TOK, D, D, "nt", c=BF16, epi=EPI_RESIDUAL)) == 2
    # without the fold the residual is an nt product like any other
    lib.vitmi_debug_gemm_rfold(0)
    assert pipe(proj_fwd()) == 2
    # a forced main loop is taken as it is; a forced 3 resolves to 1 where the fold does not exist
    for n in range(4):
        lib.vitmi_debug_reset()
        lib.vitmi_debug_gemm_pipe(n)
        assert pipe(proj_fwd()) == n
        assert pipe(desc(TOK, D, D, "nt", c=BF16, epi=EPI_RESIDUAL)) == (1 if n == 3 else n)
        assert pipe(desc(TOK, 3 * D, D, "nt")) == (1 if n == 3 else n)


def test_calls_off_the_tile_kernels_have_no_plan(lib):
    from vit_torch_amd._lib import GEMM_GENERIC
    lib.vitmi_debug_reset()
    assert plan(lib, desc(TOK, 3 * D, D, "nt", impl=GEMM_GENERIC)) == (-1, 0, 0, 0)
    assert plan(lib, desc(640, 10, 384, "nt")) == (-1, 0, 0, 0)
    out = [ctypes.c_int(0) for _ in range(4)]
    d = desc(0, 0, 0, "nt")
    assert lib.vitmi_debug_gemm_plan(ctypes.byref(d), *map(ctypes.byref, out)) == -1
