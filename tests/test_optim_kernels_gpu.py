"""The five fused optimizer kernels as direct ops.* calls against the float64 rules of tests/optim_util.py.

What a wrong kernel could get away with before: the grid-stride loops never took a second pass (2048 workgroups x 256
threads cover 524 288 elements of the scalar adam_kernel and 2 097 152 of the four-wide kernels; the largest array in
the suite had 60 k), the bf16 shadow was compared for SGD only, grad_scale was 1, every run started from zero moments at
t = 0, and the tolerance (2e-5 of max|p| at lr = 1e-3) could not see a step factor that is 1 % off.

Metric (tests/optim_util.py): state arrays by rel-to-max <= 1e-6; parameters by their UPDATE u = p_after - p_before,
max|u_gpu - u_ref| <= 2^-24 max|p_ref| + 2e-6 max|u_ref| — the rounding of the stored fp32 parameter plus ~12 fp32
roundings of the element path with a x3 margin.  A step factor that is 1e-5 off does not meet it.  The hyper-parameters
of the reference are the fp32 values the C ABI receives.  Every buffer sits between 64 sentinels on each side; the
shadow is bit-identical to the bf16 rounding of the stored parameter in every case that has one.

AdaBelief adds eps to its second state on every step (the published rule: eps enters the state), so a padding lane's
`s` is exactly float32(eps) after a step, not 0; its p, m and shadow stay exactly 0.

Worst measured values: DESIGN.md §5, "Optimizer kernels against float64"."""
import functools

import pytest
import torch

import optim_util as U

pytestmark = pytest.mark.gpu

CONFIGS = {
    "sgd": dict(rule="sgd", lr=0.05, momentum=0.9),
    "adam": dict(rule="adam", lr=0.1, b1=0.9, b2=0.999, eps=1e-8, decoupled=False),
    "adamw": dict(rule="adam", lr=0.1, b1=0.9, b2=0.999, eps=1e-8, decoupled=True),
    "adagrad": dict(rule="adagrad", lr=0.1, lr_decay=0.1, eps=1e-10),
    "adadelta": dict(rule="adadelta", lr=1.0, rho=0.9, eps=1e-3),
    # the three modes of tests/test_optim_gpu.py: (rectify, decoupled, weight decay)
    "adabelief_rect_wd0": dict(rule="adabelief", lr=0.1, b1=0.9, b2=0.999, eps=1e-16, decoupled=True, rectify=True, wd=0.0),
    "adabelief_rect": dict(rule="adabelief", lr=0.1, b1=0.9, b2=0.999, eps=1e-16, decoupled=True, rectify=True),
    "adabelief_plain": dict(rule="adabelief", lr=0.1, b1=0.9, b2=0.999, eps=1e-16, decoupled=False, rectify=False),
}
# state arrays of each rule: "first" ~ N(0, 0.1), "second" = |N| * 0.01 + 1e-4
STATES = {"sgd": ("first",), "adam": ("first", "second"), "adagrad": ("second",), "adadelta": ("second", "second"),
          "adabelief": ("first", "second")}
COUNTED = ("adam", "adagrad", "adabelief")
WD, GSCALE = 0.05, 0.125

N_PASSES = 2 * 2097152 + 4 * 256 * 5 + 3          # 4 199 427: > 2 passes of the four-wide kernels, > 8 of adam's, n % 4 == 3
N_EDGES = (1, 2, 3, 4, 5, 1023, 1024, 1027, 524289, 2097157)
N_SMALL = 4099


@pytest.fixture(scope="module")
def ops(lib):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from vit_torch_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=4)
def _noise(n, seed):
    """Four seeded N(0, 1) arrays shared (read-only) by the cases of one size."""
    g = torch.Generator("cpu").manual_seed(seed)
    return tuple(torch.randn(n, generator=g) for _ in range(4))


def _inputs(cfg, n, seed, zero_state=False):
    """(p, g, [state arrays]) as fp32 CPU tensors; never modified afterwards."""
    a, b, c, d = _noise(n, seed)
    states = []
    for kind, z in zip(STATES[cfg["rule"]], (c, d)):
        if zero_state:
            states.append(torch.full((n,), cfg.get("init", 0.0)))
        else:
            states.append(z * 0.1 if kind == "first" else z.abs() * 0.01 + 1e-4)
    return a, b, states


def _launch(ops, cfg, P, G, S, shadow, state, wd, gscale):
    r = cfg["rule"]
    if r == "sgd":
        ops.sgd_momentum(P, G, S[0], shadow, cfg["lr"], cfg["momentum"], gscale)
    elif r == "adam":
        ops.adam(P, G, S[0], S[1], shadow, state, cfg["lr"], cfg["b1"], cfg["b2"], cfg["eps"], wd, cfg["decoupled"], gscale)
    elif r == "adagrad":
        ops.adagrad(P, G, S[0], shadow, state, cfg["lr"], cfg["lr_decay"], cfg["eps"], wd, gscale)
    elif r == "adadelta":
        ops.adadelta(P, G, S[0], S[1], shadow, cfg["lr"], cfg["rho"], cfg["eps"], wd, gscale)
    else:
        ops.adabelief(P, G, S[0], S[1], shadow, state, cfg["lr"], cfg["b1"], cfg["b2"], cfg["eps"], wd, cfg["decoupled"],
                      cfg["rectify"], gscale)


def _reference(cfg, p, g, states, t, wd, gscale):
    """One step in float64 at the fp32 values of the hyper-parameters -> (p, [states])."""
    r, f = cfg["rule"], U.f32
    p, g, states = p.double(), g.double(), [s.double() for s in states]
    if r == "sgd":
        out = U.sgd(p, g, states[0], f(cfg["lr"]), f(cfg["momentum"]), f(gscale))
    elif r == "adam":
        out = U.adam(p, g, states[0], states[1], t, f(cfg["lr"]), f(cfg["b1"]), f(cfg["b2"]), f(cfg["eps"]), f(wd),
                     cfg["decoupled"], f(gscale))
    elif r == "adagrad":
        out = U.adagrad(p, g, states[0], t, f(cfg["lr"]), f(cfg["lr_decay"]), f(cfg["eps"]), f(wd), f(gscale))
    elif r == "adadelta":
        out = U.adadelta(p, g, states[0], states[1], f(cfg["lr"]), f(cfg["rho"]), f(cfg["eps"]), f(wd), f(gscale))
    else:
        out = U.adabelief(p, g, states[0], states[1], t, f(cfg["lr"]), f(cfg["b1"]), f(cfg["b2"]), f(cfg["eps"]), f(wd),
                          cfg["decoupled"], cfg["rectify"], f(gscale))
    return out[0], list(out[1:])


def _wd(cfg, wd):
    return 0.0 if cfg["rule"] == "sgd" else cfg.get("wd", wd)        # vitmi_sgd_momentum has no weight decay


class Run:
    """Guarded device buffers of one case; step() launches the kernel once."""

    def __init__(self, ops, cfg, p, g, states, tick, shadow=True, misalign=0):
        self.ops, self.cfg = ops, cfg
        mk = lambda x, m=misalign: U.Guarded(x, "cuda", m)
        self.P, self.G, self.S = mk(p), mk(g), [mk(s) for s in states]
        self.shadow = mk(torch.zeros(p.numel(), dtype=torch.bfloat16)) if shadow else None
        self.state = U.Guarded(torch.tensor([float(tick)]), "cuda") if cfg["rule"] in COUNTED else None
        self.g0 = g

    def buffers(self):
        return [b for b in (self.P, self.G, *self.S, self.shadow, self.state) if b is not None]

    def step(self, wd, gscale):
        _launch(self.ops, self.cfg, self.P.win, self.G.win, [s.win for s in self.S],
                None if self.shadow is None else self.shadow.win, None if self.state is None else self.state.win, wd, gscale)
        torch.cuda.synchronize()

    def check_frame(self, name, t):
        """Everything that holds whatever the numbers are: sentinels, the gradient, the tick, the shadow's bits."""
        for b in self.buffers():
            assert b.intact(), f"{name}: a sentinel next to a buffer of {b.win.numel()} {b.win.dtype} elements was overwritten"
        assert torch.equal(self.G.cpu(), self.g0), f"{name}: the gradient was modified"
        if self.state is not None:
            assert self.state.cpu().item() == float(t), f"{name}: state[0] = {self.state.cpu().item()} after the tick, expected {t}"
        p = self.P.cpu()
        assert torch.isfinite(p).all(), f"{name}: non-finite parameter"
        if self.shadow is not None:
            assert torch.equal(self.shadow.cpu().view(torch.int16), U.bf16_rne(p).view(torch.int16)), \
                f"{name}: shadow is not the bf16 rounding of the stored parameter"
        return p


def _check_numbers(name, p_new, p_old, p_ref, s_new, s_ref, state_tol=U.STATE_TOL, base=None):
    err, bound, umax = U.update_error(p_new, p_old, p_ref)
    serr = [U.state_error(a, b) for a, b in zip(s_new, s_ref)]
    fac = U.factor_error(p_new, p_old if base is None else base, p_ref)
    print(f"OPTK {name}: update err {err:.3e} bound {bound:.3e} ({err / bound:.2f} of it) max|u| {umax:.3g} "
          f"max|p| {p_ref.abs().max().item():.3g} factor err {fac:+.2e} states {' '.join(f'{e:.2e}' for e in serr)}")
    for i, e in enumerate(serr):
        assert torch.isfinite(s_new[i]).all() and e <= state_tol, f"{name}: state {i} rel-to-max {e:.3e} > {state_tol:.1e}"
    assert err <= bound, f"{name}: update error {err:.3e} > {bound:.3e} (max|u_ref| = {umax:.4g}, common factor off by {fac:+.2e})"


def _one_step(ops, name, cfg, n, t, seed, wd=WD, gscale=GSCALE, shadow=True, misalign=0, inputs=None):
    """One launch from non-zero state with the tick preset to t - 1, checked in full; returns the stored parameter."""
    wd = _wd(cfg, wd)
    p, g, states = inputs if inputs is not None else _inputs(cfg, n, seed)
    run = Run(ops, cfg, p, g, states, t - 1, shadow, misalign)
    run.step(wd, gscale)
    p_new = run.check_frame(name, t)
    p_ref, s_ref = _reference(cfg, p, g, states, t, wd, gscale)
    base = p.double() * (1.0 - U.f32(cfg["lr"]) * U.f32(wd)) if cfg.get("decoupled") else None
    _check_numbers(name, p_new, p, p_ref, [s.cpu() for s in run.S], s_ref, base=base)
    return p_new, [s.cpu() for s in run.S]


# ------------------------------------------------------------------------------------- more than one grid pass ---
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_more_than_two_grid_passes_with_shadow_grad_scale_and_decay(ops, name):
    _one_step(ops, f"passes {name}", CONFIGS[name], N_PASSES, U.ONE_STEP_T, seed=100)


# ---------------------------------------------------------------------------- edges of one pass and of the tail ---
@pytest.mark.parametrize("n", N_EDGES)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_edges_of_one_pass_and_of_the_tail(ops, name, n):
    _one_step(ops, f"edge {name} n={n}", CONFIGS[name], n, U.ONE_STEP_T, seed=200)


# ---------------------------------------------------------------------------------------------- step-count sweep ---
SWEEP = [(name, U.SWEEP_BETA2, t) for name in ("adam", "adamw", "adagrad", "adabelief_rect", "adabelief_plain") for t in U.SWEEP_T]
SWEEP += [("adabelief_rect", b2, t) for b2, t in U.SWEEP_EXTRA]


@pytest.mark.parametrize("name,b2,t", SWEEP)
def test_step_count_sweep(ops, name, b2, t):
    """t = 5 and 6 straddle AdaBelief's rho_t >= 5 switch (rho_5 = 4.996, rho_6 = 5.994 at beta2 = 0.999)."""
    cfg = dict(CONFIGS[name])
    if "b2" in cfg:
        cfg["b2"] = b2
    _one_step(ops, f"sweep {name} b2={b2} t={t}", cfg, N_SMALL, t, seed=300)


# ----------------------------------------------------------------------------------------------------- trajectory ---
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_twelve_steps_from_zero_state(ops, name):
    """The device tick advances on its own; fresh gradients per step; the reference iterated in float64.  The update
    metric applies to the total displacement, the state bound is multiplied by the step count.  grad_scale is 1 here
    (every one-step case has 0.125): the parameter is rounded to fp32 at each of the 12 stores while the bound holds one
    such rounding, so the displacement has to be large against max|p| for the bound to be about the step factors — the
    same reason the learning rates are large.  With these, max|u| >= 0.05 max|p|, which is asserted."""
    cfg = dict(CONFIGS[name])
    if cfg["rule"] == "adagrad":
        cfg["init"] = 0.5                      # initial_accumulator_value
    wd = _wd(cfg, WD)
    p0, _, states = _inputs(cfg, N_SMALL, 400, zero_state=True)
    run = Run(ops, cfg, p0, torch.zeros(N_SMALL), states, 0)
    run.g0 = None
    gen = torch.Generator("cpu").manual_seed(401)
    p_ref, s_ref = p0.double(), [s.double() for s in states]
    for t in range(1, U.TRAJECTORY_STEPS + 1):
        run.g0 = torch.randn(N_SMALL, generator=gen)
        run.G.win.copy_(run.g0)
        run.step(wd, 1.0)
        p_ref, s_ref = _reference(cfg, p_ref, run.g0, s_ref, t, wd, 1.0)
    p_new = run.check_frame(f"trajectory {name}", U.TRAJECTORY_STEPS)
    assert (p_ref - p0.double()).abs().max() >= 0.05 * p_ref.abs().max()
    _check_numbers(f"trajectory {name}", p_new, p0, p_ref, [s.cpu() for s in run.S], s_ref,
                   state_tol=U.STATE_TOL * U.TRAJECTORY_STEPS)


# --------------------------------------------------------------------------------------------------------- shadow ---
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_without_a_shadow_the_parameter_is_the_same_bitwise(ops, name):
    cfg = CONFIGS[name]
    for n in (1027, 524289 + 3):               # body + tail in one pass; a second pass of adam's scalar loop
        with_s, st_s = _one_step(ops, f"shadow {name} n={n}", cfg, n, U.ONE_STEP_T, seed=500)
        without, st_n = _one_step(ops, f"no shadow {name} n={n}", cfg, n, U.ONE_STEP_T, seed=500, shadow=False)
        assert torch.equal(with_s.view(torch.int32), without.view(torch.int32))
        for a, b in zip(st_s, st_n):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# -------------------------------------------------------------------------------------------------- padding lanes ---
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_padding_lanes_stay_zero(ops, name):
    """ParamPack rounds spans up: elements with p = g = state = 0, in the vector body and in the scalar tail.
    Adadelta's sqrt(0 + eps) / sqrt(0 + eps) * 0 and Adagrad's 0 / (0 + eps) are 0, not NaN."""
    cfg, n = CONFIGS[name], 2051
    p, g, states = _inputs(cfg, n, 600)
    pad = torch.zeros(n, dtype=torch.bool)
    pad[1000:1301] = True                      # starts on a vector, ends inside one
    pad[2048:] = True                          # the scalar tail
    p, g, states = p.masked_fill(pad, 0.0), g.masked_fill(pad, 0.0), [s.masked_fill(pad, 0.0) for s in states]
    wd = _wd(cfg, WD)
    run = Run(ops, cfg, p, g, states, U.ONE_STEP_T - 1)
    run.step(wd, GSCALE)
    p_new = run.check_frame(f"padding {name}", U.ONE_STEP_T)
    p_ref, s_ref = _reference(cfg, p, g, states, U.ONE_STEP_T, wd, GSCALE)
    _check_numbers(f"padding {name}", p_new, p, p_ref, [s.cpu() for s in run.S], s_ref)
    assert (p_new[pad] == 0).all() and (run.shadow.cpu()[pad].float() == 0).all()
    for i, s in enumerate(run.S):
        want = U.f32(cfg["eps"]) if (cfg["rule"] == "adabelief" and i == 1) else 0.0     # eps enters AdaBelief's s
        assert (s.cpu()[pad] == want).all(), f"padding {name}: state {i} of a padding lane is not {want}"


# --------------------------------------------------------------------------------------------- alignment contract ---
@pytest.mark.parametrize("name", sorted(k for k, c in CONFIGS.items() if c["rule"] != "adam"))
def test_a_window_off_16_byte_alignment_is_refused_and_nothing_is_written(ops, name):
    """Host-side check of the four-wide kernels' contract: nothing is launched."""
    from vit_torch_amd._lib import VitmiError
    cfg, n = CONFIGS[name], 1027
    p, g, states = _inputs(cfg, n, 700)
    for which in ("all", "p", "g", "state0"):
        run = Run(ops, cfg, p, g, states, U.ONE_STEP_T - 1, misalign=1 if which == "all" else 0)
        if which == "p":
            run.P = U.Guarded(p, "cuda", 1)
        elif which == "g":
            run.G = U.Guarded(g, "cuda", 1)
        elif which == "state0":
            run.S[0] = U.Guarded(states[0], "cuda", 1)
        assert run.P.win.data_ptr() % 16 == (4 if which in ("all", "p") else 0)
        before = [b.full.clone() for b in run.buffers()]
        with pytest.raises(VitmiError, match="16-B aligned"):
            run.step(_wd(cfg, WD), GSCALE)
        torch.cuda.synchronize()
        for b, was in zip(run.buffers(), before):
            assert torch.equal(b.full, was), f"{name} ({which} misaligned): a buffer changed although the call was refused"


@pytest.mark.parametrize("name", ["adam", "adamw"])
def test_adam_accepts_a_window_one_element_off_alignment(ops, name):
    """adam_kernel is scalar: every buffer (the shadow too, 2 B off) one element off, results and sentinels as ever."""
    for n in (5, 1027):
        _one_step(ops, f"offset {name} n={n}", CONFIGS[name], n, U.ONE_STEP_T, seed=800, misalign=1)
