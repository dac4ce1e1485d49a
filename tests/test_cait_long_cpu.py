"""The oracle's CaiT attention (oracle/cait_ref.py) against the REFERENCE's own classes at cait_S24's 384-pixel
sequence lengths: Attention_talking_head over 576 tokens and Class_Attention over 577 tokens, D = 384, 8 heads
(tests/golden/talking_heads_576.npz, class_attention_577.npz, written by tests/golden/gen_golden_cait_long.py)."""
import os

import torch

from fixture_codec import check, group, load


def _fixture(name):
    return load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))


def _against(module, f, tol_y, tol_g):
    res = module.load_state_dict(group(f, "state"), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    x = f["x"].clone().requires_grad_(True)
    y = module(x)
    check("y", y, f["y"], tol_y)
    y.backward(f["dy"])
    check("dx", x.grad, f["dx"], tol_g)
    for n, p in module.named_parameters():
        if n in ("proj_l.bias", "k.bias"):      # analytically zero (softmax ignores a per-row constant): rounding noise,
            scale = max(q.grad.abs().max().item() for q in module.parameters())      # bounded against the largest gradient
            assert p.grad.abs().max().item() <= 1e-6 * scale
            continue
        check(f"grad[{n}]", p.grad, f["grad/" + n], tol_g)


def test_oracle_talking_heads_576_matches_reference():
    from oracle.cait_ref import TalkingHeadAttention
    _against(TalkingHeadAttention(384, 8, qkv_bias=True), _fixture("talking_heads_576"), 2e-6, 1e-5)


def test_oracle_class_attention_577_matches_reference():
    from oracle.cait_ref import ClassAttention
    _against(ClassAttention(384, 8, qkv_bias=True), _fixture("class_attention_577"), 2e-6, 1e-5)
