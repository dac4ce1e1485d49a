"""engine.PackedModule, the core that ClassifierHead, XCA and LPI share, through each of the three at the smallest shapes
their kernels take: what is saved and when, the backward handed out once, a frozen input, torch's accumulation contract
(bitwise: g + g is exact in fp32), the pack after load_state_dict / a device move, the state_dict keys, the CPU refusal.
No tolerance anywhere: every comparison is between two runs of the same kernels on the same inputs."""
import pytest
import torch
import torch.nn as nn

from vit_torch_amd import LPI, XCA, VitmiError
from vit_torch_amd.head import ClassifierHead

pytestmark = pytest.mark.gpu


class _PlainXCA(nn.Module):
    def __init__(self):
        super().__init__()
        self.temperature = nn.Parameter(torch.ones(2, 1, 1))
        self.qkv = nn.Linear(64, 192, bias=False)
        self.proj = nn.Linear(64, 64)


class _PlainLPI(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(8, 8, kernel_size=3, padding=1, groups=8)
        self.act = nn.GELU()
        self.bn = nn.BatchNorm2d(8)
        self.conv2 = nn.Conv2d(8, 8, kernel_size=3, padding=1, groups=8)


def _head():
    return (ClassifierHead(nn.Linear(64, 32), nn.GELU(), nn.Linear(32, 8, bias=False)), (4, 64), (),
            nn.Sequential(nn.Linear(64, 32), nn.GELU(), nn.Linear(32, 8, bias=False)))


# name -> () -> (module, input shape, the forward's extra arguments, the plain nn.Module of the same structure)
CASES = {"head": _head}
for _dt in ("bf16", "fp32"):
    CASES[f"xca-{_dt}"] = lambda dt=_dt: (XCA(64, num_heads=2, compute_dtype=dt), (2, 5, 64), (), _PlainXCA())
    CASES[f"lpi-{_dt}"] = lambda dt=_dt: (LPI(8, compute_dtype=dt), (2, 6, 8), (2, 3), _PlainLPI())


@pytest.fixture(params=list(CASES))
def case(request, lib):
    torch.manual_seed(3)
    mod, shape, extra, plain = CASES[request.param]()
    g = torch.Generator("cpu").manual_seed(5)
    x = torch.randn(shape, generator=g)
    mod = mod.cuda().train()
    with torch.no_grad():
        dy = torch.randn(mod(x.cuda(), *extra).shape, generator=g).cuda()
    return mod, x, extra, dy, plain


def _grads(mod):
    torch.cuda.synchronize()
    return {n: p.grad.clone() for n, p in mod.named_parameters()}


def test_nothing_is_saved_without_grad(case):
    mod, x, extra, dy, _ = case
    assert mod._saved is None                       # the fixture's own forward ran under no_grad
    with torch.no_grad():
        y = mod(x.cuda().requires_grad_(True), *extra)
    assert mod._saved is None and not y.requires_grad
    mod(x.cuda(), *extra)
    assert mod._saved is not None                   # parameters that need gradients: the forward is kept


def test_second_backward_through_one_graph_is_refused(case):
    mod, x, extra, dy, _ = case
    y = mod(x.cuda().requires_grad_(True), *extra)
    y.backward(dy, retain_graph=True)
    with pytest.raises(VitmiError, match="called twice"):
        y.backward(dy)
    torch.cuda.synchronize()


def test_frozen_input_gets_no_gradient_and_the_parameters_get_theirs(case):
    mod, x, extra, dy, _ = case
    xg = x.cuda().requires_grad_(True)
    mod(xg, *extra).backward(dy)
    want = _grads(mod)
    assert xg.grad is not None
    mod.zero_grad(set_to_none=True)
    returned, inner = [], mod._backward

    def spy(dout, need_dx):
        dx = inner(dout, need_dx)
        returned.append((need_dx, dx))
        return dx
    mod._backward = spy
    xf = x.cuda()
    mod(xf, *extra).backward(dy)
    got = _grads(mod)
    assert [(need, dx is None) for need, dx in returned] == [(False, True)] and xf.grad is None
    assert got.keys() == want.keys()
    for n in want:
        assert torch.equal(got[n], want[n]), f"{n}: the gradient depends on whether the input wants one"


@pytest.mark.parametrize("set_to_none", (True, False))
def test_two_backwards_accumulate_bitwise(case, set_to_none):
    mod, x, extra, dy, _ = case
    mod(x.cuda(), *extra).backward(dy)              # .grad exists (and is the pack's own view) before zero_grad
    mod.zero_grad(set_to_none=set_to_none)
    mod(x.cuda(), *extra).backward(dy)
    first = _grads(mod)
    mod(x.cuda(), *extra).backward(dy)
    second = _grads(mod)
    for n, g in first.items():
        assert bool(g.ne(0).any()), f"{n}: zero gradient, the doubling would show nothing"
        assert torch.equal(second[n], 2 * g), f"{n}: .grad after two backwards is not twice the first"


def _pack_is_the_modules_own(mod):
    pack = mod.engine().pack
    named = list(mod.named_parameters())
    assert len(pack.params) == len(named) and all(a is b for a, (_, b) in zip(pack.params, named))
    assert pack.is_current() and (pack.shadow is not None) == bool(mod.pack_shadow)


def test_pack_follows_load_state_dict_and_device_moves(case):
    mod, x, extra, dy, plain = case
    assert list(mod.state_dict().keys()) == list(plain.state_dict().keys())
    assert [n for n, _ in mod.named_parameters()] == [n for n, _ in plain.named_parameters()]
    with torch.no_grad():
        y0 = mod(x.cuda(), *extra)
    _pack_is_the_modules_own(mod)
    mod.load_state_dict({k: v.clone() for k, v in mod.state_dict().items()})
    _pack_is_the_modules_own(mod)
    assert mod.to("cuda") is mod
    _pack_is_the_modules_own(mod)
    mod.cpu().to("cuda")                            # new parameter storage: the pack is rebuilt over it
    _pack_is_the_modules_own(mod)
    assert list(mod.state_dict().keys()) == list(plain.state_dict().keys())
    with torch.no_grad():
        assert torch.equal(mod(x.cuda(), *extra), y0)


def test_cpu_input_is_refused(case):
    mod, x, extra, dy, _ = case
    with pytest.raises(VitmiError, match="no CPU fallback"):
        mod(x, *extra)
    assert mod._saved is None
