"""The data-parallel path on a real GPU: RCCL ("nccl") in a world of ONE rank, so the bucketed
async all-reduce (identity here), its ordering against the backward's two HIP streams and the
join before the optimizer all run exactly as in the 8-GPU job.  World-size-2 semantics are
covered on CPU with gloo (test_ddp_cpu.py)."""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


from ddp_util import nccl_world_of_one  # noqa: E402,F401  (the fixture, shared with test_ddp_engines_gpu.py)


def test_bucketed_allreduce_overlapped_with_backward_matches_plain_step(nccl_world_of_one, lib):
    from vit_torch_amd import CrossEntropyLoss, FusedSGD, VisionTransformer
    from vit_torch_amd.ddp import GradReducer

    def run(with_reducer):
        torch.manual_seed(3)
        m = VisionTransformer(img_size=64, patch_size=16, embed_dim=256, depth=4, num_heads=4, num_classes=10,
                              compute_dtype="bf16", residual_dtype="auto").cuda()
        m.head = torch.nn.Linear(256, 10, bias=False).cuda()
        eng = m.engine()
        red = None
        if with_reducer:
            red = GradReducer(eng.pack, min_bucket_elems=1 << 18, force=True)
            red.broadcast_parameters(0)
            eng.reducer = red
        opt = FusedSGD(m.parameters(), lr=1e-2, momentum=0.9)
        g = torch.Generator("cpu").manual_seed(0)
        x = torch.randn(256, 3, 64, 64, generator=g).cuda()     # M = 256 * 17 rows: fast GEMM path
        y = torch.randint(0, 10, (256,), generator=g).cuda()
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = CrossEntropyLoss()(m(x), y)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        torch.cuda.synchronize()
        return losses, eng.pack.flat.clone(), red

    l0, p0, _ = run(False)
    l1, p1, red = run(True)
    assert len(red.launched) >= 3, "several buckets must have been exchanged during backward"
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1), "an all-reduce over one rank must not change the step"


def test_graphed_step_captures_the_gradient_exchange(nccl_world_of_one, lib):
    """GraphedStep with a GradReducer on the engine — the bucketed async all-reduces are
    captured inside the hipGraph (RCCL's stream joins the capture) and a replayed step equals the eager one."""
    from vit_torch_amd import CrossEntropyLoss, FusedSGD, GraphedStep, VisionTransformer
    from vit_torch_amd.ddp import GradReducer

    def make():
        torch.manual_seed(5)
        m = VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=3, num_heads=2, num_classes=10,
                              compute_dtype="bf16", residual_dtype="auto").cuda()
        m.head = torch.nn.Linear(128, 10, bias=False).cuda()
        eng = m.engine()
        eng.reducer = GradReducer(eng.pack, min_bucket_elems=1 << 16, force=True)
        return m, eng, FusedSGD(m.parameters(), lr=1e-2, momentum=0.9), CrossEntropyLoss()

    g = torch.Generator("cpu").manual_seed(0)
    data = [(torch.randn(64, 3, 32, 32, generator=g).cuda(), torch.randint(0, 10, (64,), generator=g).cuda()) for _ in range(4)]
    m, eng, opt, crit = make()
    eager = []
    for x, y in [data[0]] + data:                     # one warm-up batch, as the graphed run takes
        opt.zero_grad(); loss = crit(m(x), y); loss.backward(); opt.step()
        eager.append(loss.item())
    p_eager = eng.pack.flat.clone()
    n_buckets = len(eng.reducer.launched) // 5
    assert n_buckets >= 2

    m2, eng2, opt2, crit2 = make()
    step = GraphedStep(m2, crit2, opt2, *data[0], warmup=1)
    launched_at_capture = len(eng2.reducer.launched)
    assert launched_at_capture == 2 * n_buckets       # warm-up + capture pass each queued every bucket
    # the capture pass ran on the first batch without executing: restart from the state after the warm-up step
    graphed = [step.warm_loss.item()] + [step(x, y).item() for x, y in data]
    assert len(eng2.reducer.launched) == launched_at_capture, "replays must not go through Python's reducer again"
    assert graphed == pytest.approx(eager, rel=1e-5, abs=1e-6), (graphed, eager)
    torch.testing.assert_close(eng2.pack.flat, p_eager, rtol=1e-5, atol=1e-6)


# ---- two ranks on ONE GPU over gloo: the real multi-rank logic (parameter broadcast, bucket
# spans, SUM + grad_scale = mean) through the HIP engine and its two-stream backward.
def _two_rank_worker(rank, world, port, compute, outdir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vit_torch_amd import CrossEntropyLoss, FusedSGD, VisionTransformer
    from vit_torch_amd.ddp import GradReducer
    torch.cuda.set_device(0)
    torch.manual_seed(100 + rank)                     # deliberately different init per rank
    m = VisionTransformer(img_size=64, patch_size=16, embed_dim=256, depth=3, num_heads=4, num_classes=10,
                          compute_dtype=compute, residual_dtype="auto").cuda()
    m.head = torch.nn.Linear(256, 10, bias=False).cuda()
    eng = m.engine()
    red = GradReducer(eng.pack, min_bucket_elems=1 << 18)
    red.broadcast_parameters(0)                       # rank 0's weights everywhere
    eng.reducer = red
    opt = FusedSGD(m.parameters(), lr=1e-2, momentum=0.9, grad_scale=1.0 / world)
    g = torch.Generator("cpu").manual_seed(0)
    X = torch.randn(512, 3, 64, 64, generator=g)
    Y = torch.randint(0, 10, (512,), generator=g)
    xs, ys = X[rank * 256:(rank + 1) * 256].cuda(), Y[rank * 256:(rank + 1) * 256].cuda()
    for _ in range(2):
        opt.zero_grad()
        loss = CrossEntropyLoss()(m(xs), ys)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    # results through files: a tensor in an mp.Queue can be lost when the producer exits first
    torch.save((eng.pack.flat.detach().cpu(), len(red.launched)), os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_two_ranks_on_one_gpu_match_the_global_batch_step(lib, compute, tmp_path):
    import torch.multiprocessing as mp
    from vit_torch_amd import CrossEntropyLoss, FusedSGD, VisionTransformer
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, compute, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    got = [(r,) + tuple(torch.load(tmp_path / f"rank{r}.pt")) for r in range(2)]
    assert torch.equal(got[0][1], got[1][1]), "ranks must hold identical parameters after the exchange"
    assert got[0][2] >= 4, "several buckets per backward"
    # single process, global batch of 512, same initial weights as rank 0
    torch.manual_seed(100)
    m = VisionTransformer(img_size=64, patch_size=16, embed_dim=256, depth=3, num_heads=4, num_classes=10,
                          compute_dtype=compute, residual_dtype="auto").cuda()
    m.head = torch.nn.Linear(256, 10, bias=False).cuda()
    opt = FusedSGD(m.parameters(), lr=1e-2, momentum=0.9)
    g = torch.Generator("cpu").manual_seed(0)
    X = torch.randn(512, 3, 64, 64, generator=g).cuda()
    Y = torch.randint(0, 10, (512,), generator=g).cuda()
    for _ in range(2):
        opt.zero_grad()
        CrossEntropyLoss()(m(X), Y).backward()
        opt.step()
    want = m.engine().pack.flat.detach().cpu()
    err = (got[0][1] - want).norm() / want.norm()
    # mean of two half-batch means == global mean; fp32 differs only by summation order
    assert err < (2e-6 if compute == "fp32" else 2e-4), err


def test_bench_launches_itself_and_runs_the_rccl_path_end_to_end():
    """`python bench.py --gpus N` must start its own ranks.  One GPU here, so the
    launcher path is driven with N = 1 ranks through torch.distributed.run by calling the same
    helper, with the RCCL gradient exchange forced on (GradReducer(force=True)): the line must
    come back with n_gpus 1 and the value of a plain run."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    args = ["--steps", "3", "--warmup", "1", "--arch", "dino_vits16", "--img", "32", "--batch", "128",
            "--no-cpu-baseline", "--no-parity", "--graph", "off"]
    code = ("import sys, bench; sys.argv = ['bench.py', '--gpus', '1', '--force-ddp'] + %r; "
            "raise SystemExit(bench.self_launch(1))" % (args,))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 0
    assert d["config"]["parallelism"] == "dp1" and d["config"]["hip_graph"] is False
    # the same launcher with the exchange captured inside the HIP graph (--graph on under DDP)
    code2 = code.replace("'--graph', 'off'", "'--graph', 'on'")
    assert code2 != code
    r2 = subprocess.run([sys.executable, "-c", code2], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    d2 = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][-1])
    assert d2["config"]["hip_graph"] is True and d2["value"] > 0
    print(f"\nself-launched dp1 line: eager {d['value']:.0f} images/s, captured exchange {d2['value']:.0f} images/s "
          "(logged, not asserted: a 3-step wall-clock comparison on a shared box is not a test)")


def test_bench_two_rank_line_on_one_gpu_over_gloo():
    """The multi-rank control flow of bench.py END TO END with two real ranks: launcher -> torch.distributed.run -> warm-up,
    timed steps with the bucketed exchange, max-over-ranks time, the instrumented step (every rank must run it: it contains
    collectives — rounds 1-2 ran it on rank 0 only, which would have hung any N > 1 run), one JSON line from rank 0.
    One GPU here, so the two ranks share cuda:0 and exchange over gloo (`--dist-backend gloo --single-device`); on the
    8-GPU node the same code runs one rank per GPU over RCCL."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--dist-backend", "gloo", "--single-device", "--steps", "2", "--warmup", "1",
           "--arch", "dino_vits16", "--img", "32", "--batch", "64", "--full", "--no-cpu-baseline", "--no-parity"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0)"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 128
    assert d["value"] > 0 and d["roofline"] is not None and d["config"]["hip_graph"] is False


# ---- SURVEY §8(e) in the library: Network(ddp={'size', 'rank'}) ---------------------------------------------------------
def _net_data(n_batches=3, bs=128):
    g = torch.Generator("cpu").manual_seed(21)
    return [(torch.randn(bs, 3, 32, 32, generator=g), torch.randint(0, 10, (bs,), generator=g)) for _ in range(n_batches)]


def _net_model(seed, compute="bf16"):
    from vit_torch_amd import VisionTransformer
    torch.manual_seed(seed)
    m = VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=3, num_heads=2, num_classes=10,
                          compute_dtype=compute, residual_dtype="auto")
    m.head = torch.nn.Linear(128, 10, bias=False)
    m.apply_head = True
    return m


def test_network_with_ddp_in_a_world_of_one_equals_the_plain_network(nccl_world_of_one, lib):
    """`Network(..., ddp={'size': 1, 'rank': 0, 'force': True})` on RCCL: reducer on the engine, parameters broadcast, the
    optimizer's grad_scale 1 / world, the epoch's 2-float all-reduce — the same two epochs as without `ddp`, bit for bit."""
    from vit_torch_amd.network import Network
    train, val = _net_data(), _net_data(2)
    plain = Network(_net_model(7), opt="sgd", lr=0.02, lr_step=1, device="cuda")
    want = plain.fit(train, val, epochs=2)
    net = Network(_net_model(7), opt="sgd", lr=0.02, lr_step=1, device="cuda", ddp={"size": 1, "rank": 0, "force": True})
    assert net.model.engine().reducer is net.reducer and net.optimizer.param_groups[0]["grad_scale"] == 1.0
    got = net.fit(net.shard(train), net.shard(val), epochs=2)
    assert len(net.reducer.launched) >= 2 * len(train)
    for w, g in zip(want, got):
        assert g["train"]["loss"] == w["train"]["loss"] and g["val"]["loss"] == w["val"]["loss"]
        assert g["train"]["loss_avg"] == pytest.approx(w["train"]["loss_avg"], rel=1e-6)
        assert g["train"]["acc"] == pytest.approx(w["train"]["acc"]) and g["val"]["acc"] == pytest.approx(w["val"]["acc"])
        assert g["train"]["samples_global"] == 3 * 128
    assert torch.equal(net.model.engine().pack.flat, plain.model.engine().pack.flat)


def _two_rank_network_worker(rank, world, port, outdir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vit_torch_amd.network import Network
    torch.cuda.set_device(0)
    net = Network(_net_model(50 + rank, "fp32"), opt="sgd", lr=0.02, lr_step=1, device="cuda", ddp={"size": world, "rank": rank})
    hist = net.fit(net.shard(_net_data()), net.shard(_net_data(2)), epochs=2)
    torch.cuda.synchronize()
    torch.save((net.model.engine().pack.flat.detach().cpu(), [(h["train"]["loss_avg"], h["train"]["acc"], h["val"]["loss_avg"],
                                                               h["val"]["acc"]) for h in hist]), os.path.join(outdir, f"net{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_network_fit_two_ranks_on_one_gpu_match_the_global_batch_run(lib, tmp_path):
    """Two processes on the one GPU (gloo between them), each `Network.fit` on its half of every global batch through the
    HIP engine in fp32 mode; rank 1 starts from other weights.  Parameters and epoch figures equal the single-process run
    on the whole batches."""
    import torch.multiprocessing as mp
    from vit_torch_amd.network import Network
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_two_rank_network_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    got = [torch.load(tmp_path / f"net{r}.pt") for r in range(2)]
    assert torch.equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    ref = Network(_net_model(50, "fp32"), opt="sgd", lr=0.02, lr_step=1, device="cuda")
    want = ref.fit(_net_data(), _net_data(2), epochs=2)
    flat = ref.model.engine().pack.flat.detach().cpu()
    assert (got[0][0] - flat).norm() / flat.norm() < 5e-6
    for e in range(2):
        tl, ta, vl, va = got[0][1][e]
        assert tl == pytest.approx(want[e]["train"]["loss_avg"], rel=2e-5) and vl == pytest.approx(want[e]["val"]["loss_avg"], rel=2e-5)
        assert ta == pytest.approx(want[e]["train"]["acc"], abs=1e-9) and va == pytest.approx(want[e]["val"]["acc"], abs=1e-9)


# ---- libvitmi_comm.so: the own RCCL communicator ------------------------------------------------------------------------
def test_own_rccl_communicator_in_a_world_of_one(nccl_world_of_one, lib):
    """ncclCommInitRank through libvitmi_comm (RCCL bound from the copy PyTorch loaded), what RCCL reports about the
    communicator, the async bucket exchange ordered against the compute stream, join, broadcast, the metric all-reduce."""
    from vit_torch_amd import comm
    c = comm.default_comm()
    assert comm.default_comm() is c, "one communicator per process"
    info = c.info()
    assert info["comm_ranks"] == 1 and info["comm_rank"] == 0 and info["comm_device"] == torch.cuda.current_device()
    assert 20000 <= info["rccl_version"] < 30000
    buf = torch.arange(1 << 20, dtype=torch.float32, device="cuda")
    want = buf * 2 + 1
    buf.mul_(2)                                   # queued on the compute stream BEFORE the exchange: must be seen by it
    c.allreduce_async(buf)                        # identity over one rank, on the comm stream
    c.join()
    buf.add_(1)                                   # after the join: ordered behind the exchange
    torch.cuda.synchronize()
    assert torch.equal(buf, want)
    c.broadcast(buf, 0)
    small = torch.tensor([3.5, 2.0], device="cuda")
    c.allreduce(small)
    torch.cuda.synchronize()
    assert small.tolist() == [3.5, 2.0] and torch.equal(buf, want)
    with pytest.raises(Exception, match="fp32"):
        c.allreduce_async(buf.to(torch.bfloat16))


@pytest.mark.parametrize("transport", ["rccl", "pg"])
def test_both_transports_leave_the_step_unchanged(nccl_world_of_one, lib, transport):
    from vit_torch_amd import CrossEntropyLoss, FusedSGD, VisionTransformer
    from vit_torch_amd.ddp import GradReducer

    def run(tr):
        torch.manual_seed(3)
        m = VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=3, num_heads=2, num_classes=10,
                              compute_dtype="bf16", residual_dtype="auto").cuda()
        m.head = torch.nn.Linear(128, 10, bias=False).cuda()
        eng = m.engine()
        red = None
        if tr is not None:
            red = eng.reducer = GradReducer(eng.pack, min_bucket_elems=1 << 16, force=True, transport=tr)
            red.broadcast_parameters(0)
        opt = FusedSGD(m.parameters(), lr=1e-2, momentum=0.9)
        g = torch.Generator("cpu").manual_seed(0)
        x, y = torch.randn(64, 3, 32, 32, generator=g).cuda(), torch.randint(0, 10, (64,), generator=g).cuda()
        for _ in range(3):
            opt.zero_grad(); CrossEntropyLoss()(m(x), y).backward(); opt.step()
        torch.cuda.synchronize()
        return eng.pack.flat.clone(), red

    p0, _ = run(None)
    p1, red = run(transport)
    assert (red.comm is not None) == (transport == "rccl") and len(red.launched) >= 6
    assert red.transport_info()["transport"].startswith("libvitmi_comm" if transport == "rccl" else "torch.distributed")
    assert torch.equal(p0, p1)


def test_shared_device_flag_only_on_the_launches_right_after_a_bucket(nccl_world_of_one, lib):
    """VITMI_LAUNCH_SHARED_DEVICE on the `shared_launches` launches after each bucket's flush, not on
    every launch from the first bucket to finish()."""
    from vit_torch_amd._lib import LAUNCH_SHARED_DEVICE
    from vit_torch_amd.ddp import GradReducer
    from vit_torch_amd.packing import ParamPack
    lin = torch.nn.Linear(1024, 1024).cuda()
    pack = ParamPack(list(lin.named_parameters()), "cuda", shadow=False)
    red = GradReducer(pack, min_bucket_elems=1, force=True)
    assert red.launch_flags() == 0                               # nothing in flight yet
    red.section_ready([lin.bias])
    flags = [red.launch_flags() for _ in range(red.shared_launches + 2)]
    assert flags == [LAUNCH_SHARED_DEVICE] * red.shared_launches + [0, 0]
    red.section_ready([lin.weight])
    assert red.launch_flags() == LAUNCH_SHARED_DEVICE            # a new bucket re-arms it
    red.finish()
    assert red.launch_flags() == 0
    torch.cuda.synchronize()


def test_network_ddp_with_a_stock_torch_optimizer_scales_the_flat_gradient(nccl_world_of_one, lib):
    """`opt="torch_sgd"` has no grad_scale argument: the SUM -> mean division runs over the flat gradient buffer
    (vitmi_scale_cast in place) before `optimizer.step()`.  World of one: the factor is 1, the step must equal the plain one."""
    from vit_torch_amd.network import Network
    train = _net_data(2)
    plain = Network(_net_model(11, "fp32"), opt="torch_sgd", lr=0.02, device="cuda")
    want = plain.fit(train, None, epochs=1)
    net = Network(_net_model(11, "fp32"), opt="torch_sgd", lr=0.02, device="cuda", ddp={"size": 1, "rank": 0, "force": True})
    got = net.fit(net.shard(train), None, epochs=1)
    assert got[0]["train"]["loss"] == want[0]["train"]["loss"]
    assert torch.equal(net.model.engine().pack.flat, plain.model.engine().pack.flat)


def test_network_hip_graph_with_ddp_captures_the_exchange(nccl_world_of_one, lib):
    """`Network(hip_graph=True, ddp=...)`: the training step replays from a HIP graph that contains the bucket all-reduces on
    the own RCCL communicator (fork event / ncclAllReduce / join event as graph nodes).  Same epochs as the eager data-parallel
    Network; the reducer is not re-entered from Python during replays."""
    from vit_torch_amd.network import Network
    train = _net_data(4)
    eager = Network(_net_model(13), opt="sgd", lr=0.02, device="cuda", ddp={"size": 1, "rank": 0, "force": True})
    want = eager.fit(eager.shard(train), None, epochs=2)
    net = Network(_net_model(13), opt="sgd", lr=0.02, device="cuda", hip_graph=True, ddp={"size": 1, "rank": 0, "force": True})
    got = net.fit(net.shard(train), None, epochs=2)
    assert net._graphed is not None and net._graphed.graph is not None
    launched_after = len(net.reducer.launched)
    per_step = len(set(net.reducer.launched))
    assert launched_after <= 2 * per_step + per_step, "replays went through Python's reducer"      # warm-up + capture (+ none per replay)
    for w, g in zip(want, got):
        assert g["train"]["loss"] == pytest.approx(w["train"]["loss"], rel=1e-5, abs=1e-6)
    torch.testing.assert_close(net.model.engine().pack.flat, eager.model.engine().pack.flat, rtol=1e-5, atol=1e-6)


def test_network_linear_evaluation_with_ddp_exchanges_the_heads_gradients(nccl_world_of_one, lib):
    """Linear evaluation under `ddp` (frozen backbone + ClassifierHead, main.py:184-201): the head's gradients leave through
    the reducer after its backward (one bucket), the frozen backbone is broadcast, nothing else changes: same epoch as
    without `ddp` in a world of one."""
    from vit_torch_amd import VisionModelZoo
    from vit_torch_amd.network import Network

    def parts(seed):
        torch.manual_seed(seed)
        bb = _net_model(seed)
        bb.head = torch.nn.Identity()
        bb.apply_head = False
        for p in bb.parameters():
            p.requires_grad_(False)
        return bb, VisionModelZoo.get_classifier_head(128, [32, 10])

    train = _net_data(2)
    bb0, h0 = parts(17)
    plain = Network(h0, opt="sgd", lr=0.05, device="cuda", frozen_model_bottom=bb0)
    want = plain.fit(train, None, epochs=1)
    bb1, h1 = parts(17)
    net = Network(h1, opt="sgd", lr=0.05, device="cuda", frozen_model_bottom=bb1, ddp={"size": 1, "rank": 0, "force": True})
    got = net.fit(net.shard(train), None, epochs=1)
    assert len(net.reducer.launched) == len(train), "one bucket per step: the head's gradients"
    assert got[0]["train"]["loss"] == want[0]["train"]["loss"]
    assert torch.equal(net.model.pack.flat, plain.model.pack.flat)
