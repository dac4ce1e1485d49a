"""The engines' launch helpers and ops.py's shared argument checks without a GPU and without the library: the reducer's
launch flags are asked for once per launch that carries them (GradReducer.launch_flags() spends a credit), an unprofiled
launch is the call and nothing else, and the tensor contract / dtype code / gemm keyword checks refuse what they should."""
import types

import pytest
import torch

from vit_torch_amd import VitmiError, engine, ops
from vit_torch_amd._lib import EPI_RESIDUAL

SENTINEL = 0x40


class _Reducer:
    def __init__(self):
        self.calls = 0

    def launch_flags(self):
        self.calls += 1
        return SENTINEL


def _eng(reducer=True, split3=False, T=torch.float32):
    return types.SimpleNamespace(profile=None, split3=split3, T=T, pad_rows=False, reducer=_Reducer() if reducer else None)


def test_reducer_is_asked_once_and_only_for_a_launch_without_flags():
    eng = _eng()
    assert engine.reducer_flags(eng) == SENTINEL and eng.reducer.calls == 1
    assert engine.reducer_flags(eng, None) == SENTINEL and eng.reducer.calls == 2
    for passed in (0, 2):
        eng = _eng()
        assert engine.reducer_flags(eng, passed) == passed and eng.reducer.calls == 0
    assert engine.reducer_flags(_eng(reducer=False)) == 0
    assert engine.reducer_flags(_eng(reducer=False), 2) == 2


@pytest.mark.parametrize("split3", (False, True))
@pytest.mark.parametrize("passed", (None, 0, 2))
def test_engine_gemm_spends_one_credit_per_gemm(monkeypatch, split3, passed):
    """One launch, one question; none when the caller brought flags.  In bf16x3 mode the LayerScale residual (a GEMM, a
    scale and an add) is still ONE GEMM."""
    seen = []
    monkeypatch.setattr(ops, "gemm", lambda A, B, C, **k: seen.append(k["launch_flags"]))
    monkeypatch.setattr(ops, "gemm_split3", lambda A, B, C, **k: seen.append(k["launch_flags"]))
    monkeypatch.setattr(ops, "scale_cast", lambda *a, **k: None)
    monkeypatch.setattr(ops, "axpy", lambda *a, **k: None)
    A, B, C = torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(4, 6)
    k = {} if passed is None else {"launch_flags": passed}
    want = SENTINEL if passed is None else passed
    eng = _eng(split3=split3)
    engine.engine_gemm(eng, A, B, C, **k)
    assert seen == [want] and eng.reducer.calls == (1 if passed is None else 0)
    eng = _eng(split3=split3)
    engine.engine_gemm(eng, A, B, C, epilogue=EPI_RESIDUAL, R=torch.zeros(4, 6), C2=torch.zeros(4, 6), gamma=torch.ones(6), **k)
    assert seen == [want, want] and eng.reducer.calls == (1 if passed is None else 0)
    eng = _eng(reducer=False, split3=split3)
    engine.engine_gemm(eng, A, B, C, **k)
    assert seen[-1] == (passed or 0)


def test_unprofiled_launch_is_the_call_alone(monkeypatch):
    def no_events(*a, **k):
        raise AssertionError("an unprofiled launch made a timing event")
    monkeypatch.setattr(torch.cuda, "Event", no_events)
    eng = _eng(reducer=False)
    before = dict(vars(eng))
    calls = []
    assert engine.profiled_launch(eng, "gemm_nt", (4, 6, 8), 384.0, lambda: calls.append(1) or "out") == "out"
    assert calls == [1] and vars(eng) == before


def test_profiled_launch_brackets_the_call_and_appends_the_record(monkeypatch):
    order = []

    class Event:
        def __init__(self, enable_timing=False):
            assert enable_timing

        def record(self):
            order.append(self)

    monkeypatch.setattr(torch.cuda, "Event", Event)
    eng = _eng(reducer=False)
    eng.profile = []
    engine.profiled_launch(eng, "gemm_tn_pair", (4, 6, 8), 384.0, lambda: order.append("launch"))
    (name, shape, flops, e0, e1), = eng.profile
    assert (name, shape, flops) == ("gemm_tn_pair", (4, 6, 8), 384.0) and order == [e0, "launch", e1] and e0 is not e1


def _fake_events(monkeypatch):
    class Event:
        def __init__(self, enable_timing=False):
            pass

        def record(self):
            pass

    monkeypatch.setattr(torch.cuda, "Event", Event)


@pytest.mark.parametrize("split3, prefix", ((False, "gemm_"), (True, "gemm3_")))
@pytest.mark.parametrize("akm, bkm, form", ((True, True, "nt"), (True, False, "nn"), (False, False, "tn"), (False, True, "tt")))
def test_a_profiled_gemm_is_recorded_under_its_form_with_m_n_k_and_2mnk_flops(monkeypatch, split3, prefix, akm, bkm, form):
    """The record bench.py's roofline leg reads: A is [M, K] when k-major, else [K, M]; likewise B."""
    _fake_events(monkeypatch)
    launched = []
    monkeypatch.setattr(ops, "gemm", lambda A, B, C, **k: launched.append("gemm_"))
    monkeypatch.setattr(ops, "gemm_split3", lambda A, B, C, **k: launched.append("gemm3_"))
    M, N, K = 4, 6, 8
    A, B, C = torch.zeros((M, K) if akm else (K, M)), torch.zeros((N, K) if bkm else (K, N)), torch.zeros(M, N)
    eng = _eng(reducer=False, split3=split3)
    eng.profile = []
    engine.engine_gemm(eng, A, B, C, a_kmajor=akm, b_kmajor=bkm)
    assert launched == [prefix] and [r[:3] for r in eng.profile] == [(prefix + form, (M, N, K), 2.0 * M * N * K)]
    eng.profile = []
    engine.engine_gemm(eng, torch.zeros(M, K), torch.zeros(N, K), C)         # the defaults: both k-major
    assert [r[:3] for r in eng.profile] == [(prefix + "nt", (M, N, K), 2.0 * M * N * K)]


def test_a_paired_weight_gradient_is_one_launch_one_credit_and_one_record(monkeypatch):
    launched = []
    monkeypatch.setattr(ops, "gemm_pair_shares_a_launch", lambda *a: True)
    monkeypatch.setattr(ops, "gemm_pair", lambda *a, launch_flags: launched.append(launch_flags))
    K, (M0, M1), N = 16, (4, 12), 4
    args = (torch.zeros(K, M0, dtype=torch.bfloat16), torch.zeros(K, N, dtype=torch.bfloat16), torch.zeros(M0, N),
            torch.zeros(K, M1, dtype=torch.bfloat16), torch.zeros(K, N, dtype=torch.bfloat16), torch.zeros(M1, N))
    eng = _eng()
    monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: pytest.fail("an unprofiled launch made a timing event"))
    engine.engine_wgrad_pair(eng, *args)
    assert launched == [SENTINEL] and eng.reducer.calls == 1
    _fake_events(monkeypatch)
    eng.profile = []
    engine.engine_wgrad_pair(eng, *args)
    assert launched == [SENTINEL] * 2 and eng.reducer.calls == 2
    assert [r[:3] for r in eng.profile] == [("gemm_tn_pair", (M0 + M1, N, K), 2.0 * K * (M0 + M1) * N)]


@pytest.mark.parametrize("fault, t", (("dtype", torch.zeros(2, 3, 4, dtype=torch.float64)),
                                      ("strides", torch.zeros(2, 4, 3).transpose(1, 2)),
                                      ("count", torch.zeros(2, 3, 5))))
def test_tensor_contract_names_the_tensor_the_shape_and_what_it_got(fault, t):
    ops._contract("xca_fwd", "out", torch.zeros(2, 3, 4), torch.float32, 24, "[B, N, H*hd] = [2, 3, 4]")
    with pytest.raises(VitmiError) as e:
        ops._contract("xca_fwd", "out", t, torch.float32, 24, "[B, N, H*hd] = [2, 3, 4]")
    msg = str(e.value)
    assert "xca_fwd: out must be a contiguous torch.float32 [B, N, H*hd] = [2, 3, 4] tensor" in msg
    assert str(t.dtype) in msg and str(tuple(t.shape)) in msg


def test_dtype_code_is_minus_one_for_a_dtype_the_library_does_not_take():
    assert ops.dtype_code_or_neg(torch.float16) == -1 and ops.dtype_code_or_neg(torch.zeros(1, dtype=torch.float16)) == -1
    assert ops.dtype_code_or_neg(torch.bfloat16) == ops.BF16 == ops.dtype_code(torch.zeros(1, dtype=torch.bfloat16))
    assert ops.dtype_code_or_neg(torch.zeros(1)) == ops.F32 == ops.dtype_code(torch.zeros(1))
    with pytest.raises(TypeError, match="unsupported dtype"):
        ops.dtype_code(torch.zeros(1, dtype=torch.float16))


def test_gemm_refuses_an_unknown_keyword_before_it_loads_the_library(monkeypatch):
    def no_load():
        raise AssertionError("ops.gemm loaded the library before it looked at its keywords")
    monkeypatch.setattr(ops, "load", no_load)
    with pytest.raises(TypeError, match="a_kmajr"):
        ops.gemm(torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(4, 6), a_kmajr=False)
