"""The float64 references of tests/optim_util.py are the rules torch.optim and oracle/optim_ref.py implement: 12 steps on
float64 CPU parameters with identical injected gradients and un-rounded hyper-parameters, agreement 1e-12 rel-to-max.
And no (beta2, t) that tests/test_optim_kernels_gpu.py runs with rectify=True sits on AdaBelief's rho_t >= 5 switch."""
import pytest
import torch

import optim_util as U

N, STEPS, TOL = 257, 12, 1e-12


def _start():
    g = torch.Generator().manual_seed(11)
    return torch.randn(N, dtype=torch.float64, generator=g)


def _grads():
    g = torch.Generator().manual_seed(12)
    return [torch.randn(N, dtype=torch.float64, generator=g) for _ in range(STEPS)]


def _torch_run(make):
    q = torch.nn.Parameter(_start())
    opt = make([q])
    for gr in _grads():
        q.grad = gr.clone()
        opt.step()
    return q.data, opt.state[q]


def _close(name, got, want):
    e = U.state_error(got, want)
    assert e <= TOL, f"{name}: rel-to-max {e:.3e} > {TOL:.0e}"


def test_sgd_reference_is_torch_sgd():
    want, st = _torch_run(lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=0.9))
    p, buf = _start(), torch.zeros(N, dtype=torch.float64)
    for gr in _grads():
        p, buf = U.sgd(p, gr, buf, 0.05, 0.9)
    _close("sgd p", p, want)
    _close("sgd buf", buf, st["momentum_buffer"])


@pytest.mark.parametrize("decoupled", [False, True])
def test_adam_reference_is_torch_adam_and_adamw(decoupled):
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    want, st = _torch_run(lambda ps: cls(ps, lr=0.1, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05))
    p, m, v = _start(), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for t, gr in enumerate(_grads(), 1):
        p, m, v = U.adam(p, gr, m, v, t, 0.1, 0.9, 0.999, 1e-8, 0.05, decoupled)
    _close("adam p", p, want)
    _close("adam m", m, st["exp_avg"])
    _close("adam v", v, st["exp_avg_sq"])


def test_adagrad_reference_is_torch_adagrad():
    want, st = _torch_run(lambda ps: torch.optim.Adagrad(ps, lr=0.1, lr_decay=0.1, weight_decay=0.05, eps=1e-10,
                                                         initial_accumulator_value=0.5))
    p, s = _start(), torch.full((N,), 0.5, dtype=torch.float64)
    for t, gr in enumerate(_grads(), 1):
        p, s = U.adagrad(p, gr, s, t, 0.1, 0.1, 1e-10, 0.05)
    _close("adagrad p", p, want)
    _close("adagrad sum", s, st["sum"])


def test_adadelta_reference_is_torch_adadelta():
    want, st = _torch_run(lambda ps: torch.optim.Adadelta(ps, lr=1.0, rho=0.9, eps=1e-3, weight_decay=0.05))
    p, sq, acc = _start(), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for gr in _grads():
        p, sq, acc = U.adadelta(p, gr, sq, acc, 1.0, 0.9, 1e-3, 0.05)
    _close("adadelta p", p, want)
    _close("adadelta square_avg", sq, st["square_avg"])
    _close("adadelta acc_delta", acc, st["acc_delta"])


@pytest.mark.parametrize("rectify,decoupled,wd", [(True, True, 0.0), (True, True, 0.05), (False, False, 0.05), (True, False, 0.05)])
def test_adabelief_reference_is_the_oracle(rectify, decoupled, wd):
    from oracle.optim_ref import AdaBeliefRef
    want, st = _torch_run(lambda ps: AdaBeliefRef(ps, lr=0.1, betas=(0.9, 0.999), eps=1e-16, weight_decay=wd,
                                                  weight_decouple=decoupled, rectify=rectify))
    p, m, s = _start(), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for t, gr in enumerate(_grads(), 1):
        p, m, s = U.adabelief(p, gr, m, s, t, 0.1, 0.9, 0.999, 1e-16, wd, decoupled, rectify)
    _close("adabelief p", p, want)
    _close("adabelief m", m, st["m"])
    _close("adabelief s", s, st["s"])


def test_references_take_numpy_arrays_too():
    p, g = _start(), _grads()[0]
    m, s = 0.1 * _grads()[1], 0.01 * _grads()[2].abs() + 1e-4
    a = U.adabelief(p, g, m, s, 7, 0.1, 0.9, 0.999, 1e-16, 0.05, False, True, 0.125)
    b = U.adabelief(p.numpy(), g.numpy(), m.numpy(), s.numpy(), 7, 0.1, 0.9, 0.999, 1e-16, 0.05, False, True, 0.125)
    for x, y in zip(a, b):
        _close("numpy vs torch", torch.from_numpy(y), x)


def test_no_rectified_case_of_the_gpu_file_sits_on_the_rho_switch():
    """The switch is crossed between t = 5 and t = 6 at both beta2 the GPU file uses, and closely: rho_5 = 4.9960 at 0.999
    and 4.9598 at 0.99 (rho_t ~ t - (t^2 - 1)(1 - beta2) / 6 for small t).  A margin of 0.05, which an fp32 rho_t with its
    error of about 0.01 (1999 cancels down to 5) would need, therefore cannot be had together with t = 5, the step every
    default run passes through.  The kernel forms rho_t in double from the fp32 hyper-parameters: its error is that of
    the cancellation, rho_inf * a few dozen 2^-53 < 1e-10 at these beta2.  The margin asked here is 1e-3, 1e7 times that,
    both for the value as written and for the fp32 value the ABI gets — and the two must agree on the branch."""
    cases = U.rectified_beta2_t()
    assert (0.999, 5) in cases and (0.999, 6) in cases and (0.99, 5) in cases and (0.99, 6) in cases
    for b2, t in cases:
        rho_inf, rho_t = U.adabelief_rho(U.f32(b2), t)
        assert rho_inf * 64 * 2.0 ** -53 < 1e-10
        assert abs(rho_t - 5.0) > 1e-3, f"beta2={b2!r}, t={t}: rho_t = {rho_t:.6f} is a coin toss for the branch"
        written = U.adabelief_rho(b2, t)[1]
        assert abs(written - 5.0) > 1e-3 and (written >= 5.0) == (rho_t >= 5.0)
    for b2 in (0.999, 0.99):
        assert U.adabelief_rho(U.f32(b2), 5)[1] < 5.0 < U.adabelief_rho(U.f32(b2), 6)[1]


def test_guarded_window_is_aligned_and_bf16_rounding_is_to_nearest_even():
    for dt in (torch.float32, torch.bfloat16):
        for mis in (0, 1):
            b = U.Guarded(torch.arange(5, dtype=dt), misalign=mis)
            isz = b.win.element_size()
            assert b.win.data_ptr() % 16 == (mis * isz) % 16 and b.lo >= U.GUARD and b.intact()
            b.full[b.hi] = 0
            assert not b.intact()
    # 1 + 2^-8 is a tie between 1 and 1 + 2^-7 (even: 1); 1 + 3 * 2^-8 ties to 1 + 2^-6
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20])
    assert U.bf16_rne(x).float().tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]
