"""Float64 references of the five fused optimizer rules, and the helpers of tests/test_optim_kernels_*.py.

The rules are restated from the comments above the kernels (csrc/elementwise.hip: sgd_momentum, adam; csrc/optim.hip:
adagrad, adadelta, adabelief) and from oracle/optim_ref.py.  Every function takes numpy or torch float64 arrays, the
step count `t` AFTER the tick where the rule has one, and the hyper-parameters, and returns the new (p, state...);
nothing is updated in place.  Only operators are used (`x ** 0.5` for the square root), so both array kinds work.

What the C ABI defines is the rule at the fp32 values of the hyper-parameters it receives: the GPU tests pass every
hyper-parameter through f32() first, and the same rounded value then enters the moment updates AND the bias corrections.
The torch-parity check on the CPU passes them un-rounded (torch's Python doubles)."""
import numpy as np
import torch

GUARD = 64                 # sentinel elements on each side of a guarded window
SENTINEL = -1536.0         # exact in fp32 and in bf16

STATE_TOL = 1e-6           # rel-to-max of a state array after one step: <= 4 fp32 roundings (2.4e-7) with a x4 margin
P_ROUND = 2.0 ** -24       # rounding of the stored fp32 parameter, relative to max|p|
P_PATH = 2e-6              # the element path: <= ~12 fp32 roundings (7e-7) of the update, x3 margin

# the step counts the GPU file runs (tests/test_optim_kernels_cpu.py checks that none of them puts AdaBelief's
# rho_t >= 5 switch within the reach of an fp32 rounding)
SWEEP_T = (1, 2, 5, 6, 7, 10, 100, 1000, 100000)
SWEEP_BETA2 = 0.999
SWEEP_EXTRA = ((0.99, 5), (0.99, 6))            # (beta2, t) AdaBelief runs besides
ONE_STEP_T = 7                                  # the multi-pass, edge, shadow, padding and alignment cases: tick preset to 6
TRAJECTORY_STEPS = 12


def f32(x: float) -> float:
    """The value a `float` argument of the C ABI carries."""
    return float(np.float32(x))


def rectified_beta2_t():
    """Every (beta2, t) at which the GPU file runs AdaBelief with rectify=True."""
    out = [(SWEEP_BETA2, t) for t in SWEEP_T] + list(SWEEP_EXTRA) + [(SWEEP_BETA2, ONE_STEP_T)]
    out += [(SWEEP_BETA2, t) for t in range(1, TRAJECTORY_STEPS + 1)]
    return sorted(set(out))


def adabelief_rho(b2: float, t: int):
    """(rho_inf, rho_t) of the RAdam rectification, in float64."""
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    b2t = b2 ** float(t)
    return rho_inf, rho_inf - 2.0 * t * b2t / (1.0 - b2t)


# ---------------------------------------------------------------------------------------------------- the rules ---
def sgd(p, g, buf, lr, momentum, grad_scale=1.0):
    """buf = momentum buf + grad_scale g; p -= lr buf   (torch.optim.SGD, dampening 0, no weight decay in the kernel)"""
    buf = momentum * buf + grad_scale * g
    return p - lr * buf, buf


def adam(p, g, m, v, t, lr, b1, b2, eps, weight_decay=0.0, decoupled=True, grad_scale=1.0):
    """p *= 1 - lr wd (AdamW) | g += wd p (Adam); m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
    p -= lr/(1-b1^t) m / (sqrt(v)/sqrt(1-b2^t) + eps)"""
    g = g * grad_scale
    if decoupled:
        p = p * (1.0 - lr * weight_decay)
    else:
        g = g + weight_decay * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)
    return p - (lr / bc1) * m / (v ** 0.5 / bc2 ** 0.5 + eps), m, v


def adagrad(p, g, s, t, lr, lr_decay, eps, weight_decay=0.0, grad_scale=1.0):
    """g += wd p; clr = lr / (1 + (t-1) lr_decay); sum += g^2; p -= clr g / (sqrt(sum) + eps)"""
    g = g * grad_scale + weight_decay * p
    clr = lr / (1.0 + (t - 1) * lr_decay)
    s = s + g * g
    return p - clr * g / (s ** 0.5 + eps), s


def adadelta(p, g, sq, acc, lr, rho, eps, weight_decay=0.0, grad_scale=1.0):
    """g += wd p; sq = rho sq + (1-rho) g^2; d = sqrt(acc + eps) / sqrt(sq + eps) g; acc = rho acc + (1-rho) d^2; p -= lr d"""
    g = g * grad_scale + weight_decay * p
    sq = rho * sq + (1.0 - rho) * g * g
    d = (acc + eps) ** 0.5 / (sq + eps) ** 0.5 * g
    acc = rho * acc + (1.0 - rho) * d * d
    return p - lr * d, sq, acc


def adabelief(p, g, m, s, t, lr, b1, b2, eps, weight_decay=0.0, decoupled=True, rectify=True, grad_scale=1.0):
    """p *= 1 - lr wd | g += wd p; m = b1 m + (1-b1) g; s = b2 s + (1-b2) (g-m)^2 + eps; then
    rectified: rho_t >= 5: p -= lr r_t/(1-b1^t) m / (sqrt(s) + eps), else p -= lr/(1-b1^t) m
    not rectified: p -= lr/(1-b1^t) m / (sqrt(s)/sqrt(1-b2^t) + eps)"""
    g = g * grad_scale
    if decoupled:
        p = p * (1.0 - lr * weight_decay)
    else:
        g = g + weight_decay * p
    m = b1 * m + (1.0 - b1) * g
    r = g - m
    s = b2 * s + (1.0 - b2) * r * r + eps
    bc1, bc2 = 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)
    if not rectify:
        return p - (lr / bc1) * m / (s ** 0.5 / bc2 ** 0.5 + eps), m, s
    rho_inf, rho_t = adabelief_rho(b2, t)
    if rho_t >= 5.0:
        rt = (bc2 * (rho_t - 4.0) / (rho_inf - 4.0) * (rho_t - 2.0) / rho_t * rho_inf / (rho_inf - 2.0)) ** 0.5
        return p - (lr * rt / bc1) * m / (s ** 0.5 + eps), m, s
    return p - (lr / bc1) * m, m, s


# ------------------------------------------------------------------------------------------------------ helpers ---
class Guarded:
    """One allocation holding `values` in a 16-byte-aligned window (moved `misalign` elements off it on request) with
    at least GUARD sentinel elements on each side.  `win` is what a kernel gets; `intact()` says no sentinel changed."""

    def __init__(self, values: torch.Tensor, device="cpu", misalign: int = 0):
        values = values.contiguous()
        n, isz = values.numel(), values.element_size()
        self.full = torch.full((n + 2 * GUARD + 16 // isz + misalign,), SENTINEL, dtype=values.dtype, device=device)
        off = GUARD
        while (self.full.data_ptr() + off * isz) % 16:
            off += 1
        off += misalign
        self.lo, self.hi = off, off + n
        self.win = self.full[off:off + n]
        self.win.copy_(values)
        assert self.full.numel() - self.hi >= GUARD and self.intact()

    def intact(self) -> bool:
        return bool((self.full[:self.lo] == SENTINEL).all()) and bool((self.full[self.hi:] == SENTINEL).all())

    def cpu(self) -> torch.Tensor:
        return self.win.detach().cpu().clone()


def bf16_rne(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16, round to nearest even, on the CPU: what the shadow must hold, bit for bit."""
    return t.detach().cpu().float().to(torch.bfloat16)


def state_error(got: torch.Tensor, ref: torch.Tensor) -> float:
    """The project's rel-to-max, max|got - ref| / max|ref|, in float64."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    den = ref.abs().max().item()
    return (got - ref).abs().max().item() / (den if den else 1.0)


def update_error(p_new: torch.Tensor, p_old: torch.Tensor, p_ref: torch.Tensor):
    """(max|u_got - u_ref|, its bound 2^-24 max|p_ref| + 2e-6 max|u_ref|, max|u_ref|) with u = p_after - p_before in float64."""
    p_new, p_old, p_ref = (x.detach().cpu().double() for x in (p_new, p_old, p_ref))
    u_got, u_ref = p_new - p_old, p_ref - p_old
    umax = u_ref.abs().max().item()
    return (u_got - u_ref).abs().max().item(), P_ROUND * p_ref.abs().max().item() + P_PATH * umax, umax


def factor_error(p_new: torch.Tensor, p_old: torch.Tensor, p_ref: torch.Tensor) -> float:
    """Least-squares c of u_got = (1 + c) u_ref: the relative error of a factor common to the whole update (the step
    factor, where no decoupled decay adds a second term).  A measurement, not a bound."""
    p_new, p_old, p_ref = (x.detach().cpu().double() for x in (p_new, p_old, p_ref))
    u_got, u_ref = p_new - p_old, p_ref - p_old
    return float(((u_got - u_ref) * u_ref).sum() / (u_ref * u_ref).sum())
