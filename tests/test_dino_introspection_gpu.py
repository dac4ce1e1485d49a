"""VisionTransformer.get_last_selfattention / get_intermediate_layers: upstream DINO's two other public methods on the HIP
path, against the float64 oracle (oracle/vit_ref.py, depth 2, weights from seeded_init_ copied by load_state_dict).

  * get_last_selfattention(x): the last block's softmax((q k^T) * scale), fp32 [B, H, N, N];
  * get_intermediate_layers(x, n): [norm(x) after each of the last n blocks], oldest first, fp32 [B, N, D];
at dino_vits16 and dino_vitb8 dims, 224 px (N = 197 / 785), 96 px (stored 224-grid pos_embed resampled) and a
non-square 224x160 input, in every compute mode.  Plus: the cls_only_last_block option does not change either output
(and they run at N = 785, where that option's forward refuses), PatchRows input equals NCHW input, the CLS row of the
last layer is forward's output, forward is unchanged after the methods ran, and both refuse to build an autograd graph.

Error metric: max |got - want| / max |want| (util.rel_err) per tensor; for P the plain max |got - want| (P lies in
[0, 1]).  Bounds, each 2-3x the largest value measured on an MI355X (in brackets; every check prints its error beside
its bound with -s):
  * fp32 [P 4.3e-8, layers 2.8e-6]: FP32_P = 1e-7, FP32_L = 8e-6 (the project's fp32 parity level, ~1e-5).
  * bf16x3, every product as three bf16 products [P 2.3e-7, layers 8.9e-6]: X3_P = 6e-7, X3_L = 2.5e-5.
  * bf16 operands, fp32 residual stream [P 1.3e-4, layers 5.2e-3]: BF_P = 3e-4, BF_L = 1.3e-2.
  * bf16 operands, bf16 residual stream [P 1.7e-4, layers 9.0e-3]: BB_P = 4e-4, BB_L = 2.2e-2.
"""
import pytest
import torch

from util import rel_err

pytestmark = pytest.mark.gpu

F64 = torch.float64
FP32_P, FP32_L = 1e-7, 8e-6
X3_P, X3_L = 6e-7, 2.5e-5
BF_P, BF_L = 3e-4, 1.3e-2
BB_P, BB_L = 4e-4, 2.2e-2
BOUNDS = {("fp32", "fp32"): (FP32_P, FP32_L), ("bf16x3", "fp32"): (X3_P, X3_L),
          ("bf16", "fp32"): (BF_P, BF_L), ("bf16", "bf16"): (BB_P, BB_L)}
DIMS = {"vits16": (16, 384, 6), "vitb8": (8, 768, 12)}
CONFIGS = [("vits16", 224, 224), ("vitb8", 224, 224), ("vitb8", 96, 96), ("vits16", 224, 160)]
NS = (0, 1, 2, 5)


@pytest.fixture(autouse=True)
def _built(lib):
    pass


def models(dims, compute="fp32", residual="fp32", depth=2, **kw):
    from oracle import vit_ref
    from vit_torch_amd import VisionTransformer
    p, d, h = DIMS[dims]
    ref = vit_ref.VisionTransformer(img_size=224, patch_size=p, embed_dim=d, depth=depth, num_heads=h)
    vit_ref.seeded_init_(ref, 1)
    m = VisionTransformer(img_size=224, patch_size=p, embed_dim=d, depth=depth, num_heads=h, compute_dtype=compute,
                          residual_dtype=residual, **kw)
    res = m.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return ref.double(), m.cuda()


def image(B, Hh, W, seed=3):
    return torch.randn(B, 3, Hh, W, generator=torch.Generator("cpu").manual_seed(seed))


@torch.no_grad()
def oracle(ref, x):
    """float64: (last block's softmax [B, H, N, N], [norm(x) after each block])."""
    t = ref.prepare_tokens(x.double())
    layers = []
    for i, blk in enumerate(ref.blocks):
        if i == len(ref.blocks) - 1:
            a = blk.attn
            B, N, C = t.shape
            qkv = a.qkv(blk.norm1(t)).reshape(B, N, 3, a.num_heads, C // a.num_heads).permute(2, 0, 3, 1, 4)
            P = ((qkv[0] @ qkv[1].transpose(-2, -1)) * a.scale).softmax(dim=-1)
        t = blk(t)
        layers.append(ref.norm(t))
    return P, layers


_ORACLE = {}


def oracle_for(dims, Hh, W):
    key = (dims, Hh, W)
    if key not in _ORACLE:
        ref, _ = models(dims)
        _ORACLE[key] = oracle(ref, image(2, Hh, W))
    return _ORACLE[key]


@pytest.mark.parametrize("compute,residual", list(BOUNDS), ids=[f"{c}-res{r}" for c, r in BOUNDS])
@pytest.mark.parametrize("dims,Hh,W", CONFIGS, ids=[f"{d}-{h}x{w}" for d, h, w in CONFIGS])
def test_against_float64_oracle(dims, Hh, W, compute, residual):
    P_tol, L_tol = BOUNDS[(compute, residual)]
    P64, layers64 = oracle_for(dims, Hh, W)
    _, m = models(dims, compute, residual)
    x = image(2, Hh, W).cuda()
    with torch.no_grad():
        P = m.get_last_selfattention(x)
        assert P.dtype == torch.float32 and tuple(P.shape) == tuple(P64.shape) and P.is_contiguous()
        e = (P.double().cpu() - P64).abs().max().item()
        print(f"\n  {dims} {Hh}x{W} {compute}/res {residual}: P {e:.2e} (bound {P_tol:.0e})", end="")
        assert torch.isfinite(P).all() and e <= P_tol, f"P: {e:.3e} > {P_tol:.1e}"
        for n in NS:
            out = m.get_intermediate_layers(x, n)
            assert isinstance(out, list) and len(out) == min(n, len(layers64))
            want = layers64[len(layers64) - len(out):]
            errs = []
            for got, w in zip(out, want):
                assert got.dtype == torch.float32 and tuple(got.shape) == tuple(w.shape)
                errs.append(rel_err(got, w))
            if errs:
                print(f", n={n}: layers {max(errs):.2e} (bound {L_tol:.0e})", end="")
                assert max(errs) <= L_tol, f"n = {n}: {max(errs):.3e} > {L_tol:.1e}"
        outs = m.get_intermediate_layers(x, 2)
        assert outs[0].data_ptr() != outs[1].data_ptr()


@pytest.mark.parametrize("side", [224, 448], ids=["N197", "N785"])
def test_cls_only_last_block_gives_the_same_tensors(side):
    _, m = models("vits16", "bf16", "fp32")
    _, mc = models("vits16", "bf16", "fp32", cls_only_last_block=True)
    x = image(2, side, side).cuda()
    with torch.no_grad():
        a, b = m.get_last_selfattention(x), mc.get_last_selfattention(x)
        assert torch.equal(a, b), f"P differs by {(a - b).abs().max().item():.3e}"
        la, lb = m.get_intermediate_layers(x, 2), mc.get_intermediate_layers(x, 2)
        for u, v in zip(la, lb):
            assert torch.equal(u, v), f"layers differ by {(u - v).abs().max().item():.3e}"
        if side == 448:
            from vit_torch_amd._lib import VitmiError
            with pytest.raises(VitmiError, match="cls_only_last_block"):
                mc(x)                                          # forward keeps refusing, as before


def test_patch_rows_input_equals_image_input():
    from vit_torch_amd.data import NORM, DeviceAugment
    _, m = models("vits16", "bf16", "fp32")
    img = torch.randint(0, 256, (2, 224, 224, 3), generator=torch.Generator("cpu").manual_seed(4),
                        dtype=torch.uint8).cuda()
    aug = DeviceAugment(224, **NORM["stl10"], train=False)
    x, rows = aug(img), aug.patch_rows(img, 16)
    with torch.no_grad():
        assert torch.equal(m.get_last_selfattention(x), m.get_last_selfattention(rows))
        for u, v in zip(m.get_intermediate_layers(x, 2), m.get_intermediate_layers(rows, 2)):
            assert torch.equal(u, v)


@pytest.mark.parametrize("compute", ["bf16", "fp32"])
def test_last_layer_cls_row_is_forward_and_forward_is_unchanged(compute):
    _, m = models("vits16", compute, "fp32")
    x = image(3, 224, 224).cuda()
    with torch.no_grad():
        before = m(x)
        P = m.get_last_selfattention(x)
        last = m.get_intermediate_layers(x, 1)[0]
        after = m(x)
    assert P.shape[-1] == 197
    assert torch.equal(before, after), "forward changed after the introspection methods ran"
    e = rel_err(last[:, 0], before)
    print(f"\n  {compute}: CLS row of get_intermediate_layers vs forward {e:.2e} (bound 1e-6)", end="")
    assert e <= 1e-6


def test_refuses_under_autograd_and_runs_under_no_grad():
    from vit_torch_amd._lib import VitmiError
    _, m = models("vits16", "bf16", "fp32")
    x = image(1, 224, 224).cuda()
    with pytest.raises(VitmiError, match="no_grad"):
        m.get_last_selfattention(x)
    with pytest.raises(VitmiError, match="no_grad"):
        m.get_intermediate_layers(x, 1)
    with torch.no_grad():
        assert m.get_last_selfattention(x).shape == (1, 6, 197, 197)
        assert len(m.get_intermediate_layers(x, 1)) == 1
    m.requires_grad_(False)                                    # a frozen backbone needs no no_grad
    assert m.get_intermediate_layers(x, 3)[0].shape == (1, 197, 384)
