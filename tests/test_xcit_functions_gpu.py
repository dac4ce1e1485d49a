"""XCiT's module kernels as functions over a parameter pack (`xcit.<name>_forward` / `<name>_backward`): run against ONE
`ParamPack` that holds the parameters of two module copies, they give the bits the two modules give through autograd on
their own packs.

Both sides run the same kernels on the same inputs and shapes, and a parameter starts on a 256-byte boundary in either pack
(`packing.ALIGN`), so every comparison is `torch.equal`: outputs, dx, every parameter gradient (`pack.g(p)` against the
module's `p.grad`), the batch-norm running buffers and `num_batches_tracked`.  A difference would mean that a result depends
on an address.  Shapes are the smallest the kernels take.
"""
import copy

import pytest
import torch
import torch.nn as nn

from vit_torch_amd import XCA, LPI, ClassAttentionBlock, ConvPatchEmbed, PositionalEncodingFourier, XCABlock, xcit
from vit_torch_amd.packing import ParamPack

pytestmark = pytest.mark.gpu
MODES = pytest.mark.parametrize("mode", ["fp32", "bf16"])

# name: (constructor, input shape, the functions' extra arguments, the module's extra arguments)
CASES = {
    "xca": (lambda mode: XCA(64, num_heads=2, qkv_bias=True, compute_dtype=mode), (2, 5, 64), (), ()),
    "lpi": (lambda mode: LPI(8, compute_dtype=mode), (2, 6, 8), (2, 3), (2, 3)),
    "conv_patch_embed": (lambda mode: ConvPatchEmbed(32, 16, embed_dim=64, compute_dtype=mode), (2, 3, 32, 32), (), ()),
    "posfourier": (lambda mode: PositionalEncodingFourier(dim=64, compute_dtype=mode), (2, 15, 64), (3, 5), (3, 5)),
    "class_attention_block": (lambda mode: ClassAttentionBlock(64, 2, qkv_bias=True, eta=1.0, tokens_norm=False,
                                                               compute_dtype=mode), (2, 5, 64), (), (2, 2)),
    "class_attention_block-tokens_norm": (lambda mode: ClassAttentionBlock(64, 2, qkv_bias=True, eta=1.0, tokens_norm=True,
                                                                           compute_dtype=mode), (2, 5, 64), (), (2, 2)),
    "xcablock": (lambda mode: XCABlock(64, 2, mlp_ratio=2, qkv_bias=True, eta=1.0, compute_dtype=mode), (2, 15, 64), (3, 5),
                 (3, 5)),
}


def seeded(m, seed):
    """every parameter and running statistic moved off its initial value by seeded noise"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.add_(0.1 * torch.randn(b.shape, generator=g))
            elif n.endswith("running_var"):
                b.add_(0.5 * torch.rand(b.shape, generator=g))
    return m


def setup(name, mode):
    """two differently seeded modules on the device, their deep copies in one ModuleList, ONE pack over the copies' parameters,
    and the function pair"""
    mods = [seeded(CASES[name][0](mode), s) for s in (1, 2)]
    holder = nn.ModuleList(copy.deepcopy(mods)).cuda().train()
    mods = [m.cuda().train() for m in mods]
    pack = ParamPack(list(holder.named_parameters()), torch.device("cuda"), shadow=mode == "bf16")
    pack.refresh_shadow()
    base = name.split("-")[0]
    return mods, holder, pack, getattr(xcit, base + "_forward"), getattr(xcit, base + "_backward")


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def tokens(out):
    return out[0] if isinstance(out, tuple) else out              # ConvPatchEmbed.forward returns (tokens, grid)


def assert_same_state(mods, holder, pack):
    for m, h in zip(mods, holder):
        for (n, p), (_, q) in zip(m.named_parameters(), h.named_parameters()):
            assert p.grad is not None and torch.equal(pack.g(q), p.grad), f"grad {n}"
        for (n, b), (_, c) in zip(m.named_buffers(), h.named_buffers()):
            assert torch.equal(b, c), f"buffer {n}"


@MODES
@pytest.mark.parametrize("name", list(CASES))
def test_functions_on_a_shared_pack_give_the_modules_bits(name, mode):
    _, shape, extra, mextra = CASES[name]
    mods, holder, pack, fwd, bwd = setup(name, mode)
    image = name == "conv_patch_embed"                                # the image gets no gradient
    for i, (m, h) in enumerate(zip(mods, holder)):
        x = randn(shape, 10 + i)
        out, saved = fwd(pack, h, x, *extra)
        dout = randn(out.shape, 20 + i)
        dx = bwd(pack, h, saved, dout, need_dx=not image)
        xm = x.clone().requires_grad_(not image)
        want = tokens(m(xm, *mextra))
        want.backward(dout)
        assert out.dtype == want.dtype and torch.equal(out, want), f"out of copy {i}"
        assert (dx is None and xm.grad is None) if image else torch.equal(dx, xm.grad), f"dx of copy {i}"
    torch.cuda.synchronize()
    assert_same_state(mods, holder, pack)
    # eval mode, nothing kept
    x = randn(shape, 30)
    out, saved = fwd(pack, holder[1].eval(), x, *extra, save=False)
    with torch.no_grad():
        want = tokens(mods[1].eval()(x, *mextra))
    assert saved is None and torch.equal(out, want)
    assert_same_state(mods, holder, pack)                          # eval moved no buffer on either side


@MODES
def test_two_chained_blocks_keep_their_forwards_apart(mode):
    """block 1 reads block 0's output and the backward runs in reverse, block 0's saved forward held while block 1 runs: what
    a model's engine does, and what one `_saved` slot per pack could not"""
    _, shape, extra, _ = CASES["xcablock"]
    mods, holder, pack, fwd, bwd = setup("xcablock", mode)
    x, dout = randn(shape, 40), randn(shape, 41)
    y0, s0 = fwd(pack, holder[0], x, *extra)
    y1, s1 = fwd(pack, holder[1], y0, *extra)
    dx = bwd(pack, holder[0], s0, bwd(pack, holder[1], s1, dout))
    xm = x.clone().requires_grad_(True)
    want = mods[1](mods[0](xm, *extra), *extra)
    want.backward(dout)
    torch.cuda.synchronize()
    assert torch.equal(y1, want) and torch.equal(dx, xm.grad)
    assert_same_state(mods, holder, pack)
