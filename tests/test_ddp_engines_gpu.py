"""The gradient exchange under every engine: VitEngine (also its CLS-only last block), CaitEngine, SwinEngine (two
stages, so PatchMerging) and the stand-alone ClassifierHead on a frozen backbone, each in fp32 and in bf16.

What decides whether replicas stay equal is WHEN a section of the flat gradient buffer is announced (`_ready`) and WHAT
its span covers: many gradients are written by a later block's LayerNorm backward (`gsum=`) or by the deferred
FoldQueue, and a section that leaves too early makes every rank step on another gradient without any error.  Every
check here is an equality, because nothing that is compared has a rounding of its own:

A. World of one (RCCL, `force=True`).  The all-reduce is the identity, so a copy of each bucket taken at its hand-over
   (`RecordingReducer`) must EQUAL what its range holds when the backward is over: a late write or a span into an
   unfinished neighbour breaks exactly that.  The buckets tile the pack, there are as many as the model's depths imply,
   and the whole buffer EQUALS that of the same backward without a reducer (the project's rule: an exchange over one
   rank does not change the step).  One planted fault (a Swin block announced one section early) shows that the
   snapshot check bites.
B. Two ranks on the one GPU over gloo, one launch for all cases.  Per rank: L = the gradient without a reducer, S = the
   snapshots with one, E = the buffer after the exchange.  S == L (the reducer and its shared-device launch flag
   change no bit), and E_0 == E_1 == S_0 + S_1: over two ranks each element of the SUM is ONE fp32 addition, which
   is commutative and correctly rounded whatever algorithm gloo runs, so there is no tolerance.  Then `Network`:
   the fused optimizer's grad_scale 1/2, the stock optimizer's in-place SUM -> mean pass at a factor other than 1
   (x 0.5 is exact), and the reducer following the model to a rebuilt engine / a rebuilt head pack.
C. World of one (RCCL): `Network(hip_graph=True, ddp=...)` exchanges again, over the new pack, when a new GraphedStep
   is built after an engine rebuild.
"""
import pytest
import torch

from ddp_util import (COMPUTES, MODELS, RecordingReducer, assemble, assert_spans_tile, backward_once, build_case,
                      check_snapshots, check_tiling, nccl_world_of_one, pack_of, ready_calls, record, run_ranks,  # noqa: F401
                      shard)

pytestmark = pytest.mark.gpu


# ---- A: world of one ----------------------------------------------------------------------------------------------------
_PLAIN = {}


def _plain_gradient(name, compute):
    """The flat gradient of the case's backward with no reducer: computed once, shared, left unchanged."""
    key = (name, compute)
    if key not in _PLAIN:
        m, bottom = build_case(name, compute, seed=11)
        _PLAIN[key] = backward_once(m, bottom, *shard(name, 0)).grad.clone()
    return _PLAIN[key]


@pytest.mark.parametrize("min_bucket", [1, 1 << 16])
@pytest.mark.parametrize("compute", COMPUTES)
@pytest.mark.parametrize("name", MODELS)
def test_every_bucket_leaves_final_and_the_buckets_tile_the_pack(nccl_world_of_one, lib, name, compute, min_bucket):
    """`min_bucket` 1: every announced section is a bucket of its own; 1 << 16: adjacent sections merge."""
    want = _plain_gradient(name, compute)
    m, bottom = build_case(name, compute, seed=11)
    red = RecordingReducer(pack_of(m), min_bucket_elems=min_bucket, force=True)
    pack = backward_once(m, bottom, *shard(name, 0), reducer=red)
    print(f"\nbuckets[{name}, {compute}, min_bucket_elems={min_bucket}]: {len(red.launched)} "
          f"(sections announced: {ready_calls(name, m)})")
    check_tiling(red, pack)
    if min_bucket == 1:
        assert len(red.launched) >= ready_calls(name, m)
    check_snapshots(red, pack)
    assert torch.equal(pack.grad, want), "an exchange over one rank must not change the gradients"


def test_a_block_announced_one_section_early_trips_the_snapshot_check(nccl_world_of_one, lib):
    """Planted fault: block i's `_ready` also announces block i - 1 of its stage, whose own gradients are not written
    yet.  The snapshot of that bucket then differs from what its range holds in the end."""
    m, _ = build_case("swin", "bf16", seed=11)
    eng = m.engine()
    before = {}
    for layer in m.layers:
        blocks = list(layer.blocks)
        before.update({id(b): a for a, b in zip(blocks, blocks[1:])})
    honest = eng._ready

    def early(*mods):
        extra = [before[id(o)] for o in mods if id(o) in before]
        honest(*mods, *extra)

    eng._ready = early
    red = RecordingReducer(eng.pack, min_bucket_elems=1, force=True)
    pack = backward_once(m, None, *shard("swin", 0), reducer=red)
    with pytest.raises(AssertionError, match="left before its gradients were final"):
        check_snapshots(red, pack)


# ---- B: two ranks on one GPU over gloo ----------------------------------------------------------------------------------
NET_COMPUTE = "bf16"


def _after_step(net, red0=None):
    """What the parent needs of a Network after a step: the recorded buckets, the gradient buffer, the parameters."""
    torch.cuda.synchronize()
    eng = net.model.engine()
    pack, red = eng.pack, net.reducer
    rec = isinstance(red, RecordingReducer)
    return dict(attached=eng.reducer is red, on_pack=red.pack is pack, fresh=red is not red0, recording=rec,
                spans=list(red.launched), total=pack.total, S=assemble(red, pack.total).cpu() if rec and red.snaps else None,
                G=pack.grad.cpu(), params=pack.flat.cpu(),
                grad_scale=net.optimizer.param_groups[0].get("grad_scale"))


def _two_rank_worker(rank, world):
    from vit_torch_amd.ddp import GradReducer
    from vit_torch_amd.network import Network
    torch.cuda.set_device(0)
    out = {}
    for name in MODELS:
        for compute in COMPUTES:
            m, bottom = build_case(name, compute, seed=100 + rank)       # every rank starts from other weights
            pack = pack_of(m)
            GradReducer(pack).broadcast_parameters(0)
            x, y = shard(name, rank)
            L = backward_once(m, bottom, x, y).grad.cpu()
            red = RecordingReducer(pack, min_bucket_elems=1)
            backward_once(m, bottom, x, y, reducer=red)
            out[name, compute] = dict(params=pack.flat.cpu(), L=L, S=assemble(red, pack.total).cpu(), E=pack.grad.cpu(),
                                      spans=list(red.launched), total=pack.total)
            m.engine().reducer = None

    ddp = {"size": world, "rank": rank}
    for opt in ("sgd", "torch_sgd"):
        m, _ = build_case("vit", NET_COMPUTE, seed=200 + rank)
        net = Network(m, opt=opt, lr=0.02, device="cuda", ddp=ddp)
        record(net)
        net.run_one_epoch([shard("vit", rank)])
        out["net", opt] = _after_step(net)

    # the engine is rebuilt between two steps, as after a checkpoint load
    m, _ = build_case("swin", NET_COMPUTE, seed=300 + rank)
    net = Network(m, opt="sgd", lr=0.02, device="cuda", ddp=ddp)
    first = record(net)
    net.run_one_epoch([shard("swin", rank)])
    net.model._engine = None
    net.run_one_epoch([shard("swin", rank)])
    out["rebuild", "swin"] = _after_step(net, first)

    # the head's pack is rebuilt between two steps: every parameter gets a new storage, as a move between devices does
    h, bottom = build_case("head", NET_COMPUTE, seed=400 + rank)
    net = Network(h, opt="sgd", lr=0.02, device="cuda", frozen_model_bottom=bottom, ddp=ddp)
    first = record(net)
    net.run_one_epoch([shard("head", rank)])
    for p in h.parameters():
        p.data = p.data.clone()
    net.run_one_epoch([shard("head", rank)])
    out["rebuild", "head"] = _after_step(net, first)
    return out


def test_two_ranks_exchange_the_gradients_of_every_engine(lib, tmp_path):
    """One launch of two ranks for all cases of section B (module docstring).

    Wall time on the MI355X: 4.4 s, next to 6.2 s of test_ddp_gpu.py's
    test_two_ranks_on_one_gpu_match_the_global_batch_step[fp32] in the same run: one launch is kept."""
    r0, r1 = run_ranks(_two_rank_worker, 2, (), tmp_path, limit_s=420)
    for name in MODELS:
        for compute in COMPUTES:
            a, b = r0[name, compute], r1[name, compute]
            where = f"{name}, {compute}"
            assert torch.equal(a["params"], b["params"]), f"{where}: parameters differ after the broadcast"
            for r in (a, b):
                assert_spans_tile(r["spans"], r["total"])
            assert not torch.equal(a["L"], b["L"]), f"{where}: the two shards give one gradient: the case proves nothing"
            same = [torch.equal(r["S"], r["L"]) for r in (a, b)]
            print(f"\ntwo ranks[{where}]: {len(a['spans'])} buckets, S_r == L_r: {same}")
            want = a["S"] + b["S"]
            assert torch.equal(a["E"], b["E"]), f"{where}: the ranks hold different gradients after the exchange"
            assert torch.equal(a["E"], want), f"{where}: the exchanged gradient is not the sum of what the ranks handed over"
            assert all(same), f"{where}: a reducer on the engine changes what a rank computes (S_r == L_r: {same})"

    def exchanged(key, factor):
        a, b = r0[key], r1[key]
        for r in (a, b):
            assert r["attached"] and r["on_pack"] and r["recording"], \
                f"{key}: the model's engine / head does not hold the Network's reducer over its current pack: {r['attached'], r['on_pack']}"
            assert r["S"] is not None, f"{key}: no bucket left"
            assert_spans_tile(r["spans"], r["total"])
        want = (a["S"] + b["S"]) * factor
        assert torch.equal(a["G"], want) and torch.equal(b["G"], want), f"{key}: the gradient buffer is not the ranks' sum x {factor}"
        assert torch.equal(a["params"], b["params"]), f"{key}: the ranks' parameters differ after the step"
        return a, b

    a, b = exchanged(("net", "sgd"), 1.0)                 # the fused optimizer takes the mean itself
    assert a["grad_scale"] == b["grad_scale"] == 0.5
    exchanged(("net", "torch_sgd"), 0.5)                  # the in-place SUM -> mean pass; x 0.5 is exact
    for what in ("swin", "head"):
        a, b = exchanged(("rebuild", what), 1.0)
        assert a["fresh"] and b["fresh"] and a["grad_scale"] == 0.5


# ---- C: a new captured step after a rebuild ------------------------------------------------------------------------------
def test_a_new_graphed_step_after_an_engine_rebuild_exchanges_again(nccl_world_of_one, lib):
    from vit_torch_amd.network import Network
    m, _ = build_case("vit", "bf16", seed=5)
    net = Network(m, opt="sgd", lr=0.02, device="cuda", hip_graph=True, ddp={"size": 1, "rank": 0, "force": True})
    batches = [shard("vit", 0), shard("vit", 1)]
    net.run_one_epoch(batches)                            # warm-up step + capture on the first batch, a replay on the second
    first = net.reducer
    assert net._graphed.graph is not None and len(first.launched) >= 2
    net._graphed.close()
    net._graphed = None
    net.model._engine = None                              # what a checkpoint load does
    net.run_one_epoch(batches)
    torch.cuda.synchronize()
    eng = net.model.engine()
    assert net._graphed.graph is not None
    assert eng.reducer is net.reducer and net.reducer.pack is eng.pack and net.reducer is not first
    per_step = sorted(set(net.reducer.launched))
    assert_spans_tile(per_step, eng.pack.total)
    assert len(net.reducer.launched) == 2 * len(per_step), "the warm-up step and the capture pass each queue every bucket"
