"""Shared pieces of the data-parallel tests (test_ddp_gpu.py, test_ddp_engines_gpu.py, test_ddp_cpu.py).

* `run_ranks`: `world` fresh child processes (spawn) that meet in one torch.distributed job and hand their results
  back through files.
* `RecordingReducer`: a GradReducer that keeps a copy of every bucket as this rank hands it over.
* `check_tiling` / `check_snapshots` / `assemble`: what one backward's buckets must satisfy.
* `nccl_world_of_one`: the RCCL process group of one rank that the single-GPU tests run in.
* the tiny models the engine tests run (`MODELS`, `build_case`, `shard`, `backward_once`).

Nothing here needs a GPU to be imported.
"""
import datetime
import os
import socket
import sys
import time
import traceback

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from vit_torch_amd.ddp import GradReducer  # noqa: E402


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def nccl_world_of_one():
    import torch.distributed as dist
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(free_port())
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


# ---- ranks as child processes -------------------------------------------------------------------------------------------
COLLECTIVE_TIMEOUT_S = 120      # a rank whose peer died leaves its collective by itself after this long


def _rank_main(worker, rank, world, port, backend, args, outdir):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group(backend, rank=rank, world_size=world,
                                timeout=datetime.timedelta(seconds=COLLECTIVE_TIMEOUT_S))
        result = worker(rank, world, *args)
        # results through files: a tensor in an mp.Queue can be lost when the producer exits first
        torch.save(result, os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        with open(os.path.join(outdir, f"rank{rank}.err"), "w") as f:
            f.write(traceback.format_exc())
        os._exit(1)             # no atexit handler of a half-initialised job may wait for the peer


def run_ranks(worker, world, args, outdir, backend="gloo", limit_s=300):
    """`worker(rank, world, *args)` in `world` fresh processes of one torch.distributed job; returns the workers'
    return values by rank.  A child that is still alive `limit_s` seconds after the start is killed and the test
    fails; a child that raised fails the test with its traceback.  One attempt, no retries."""
    import torch.multiprocessing as mp
    assert world <= 3, "at most three processes hold the GPU at once"
    outdir = str(outdir)
    ctx = mp.get_context("spawn")
    port = free_port()
    procs = [ctx.Process(target=_rank_main, args=(worker, r, world, port, backend, tuple(args), outdir)) for r in range(world)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + limit_s
    for p in procs:
        p.join(max(0.0, deadline - time.monotonic()))
    hung = [r for r, p in enumerate(procs) if p.is_alive()]
    for r in hung:
        procs[r].kill()
        procs[r].join()
    errors = []
    for r in range(world):
        path = os.path.join(outdir, f"rank{r}.err")
        if os.path.exists(path):
            with open(path) as f:
                errors.append(f"--- rank {r} ---\n{f.read()}")
    if hung:
        pytest.fail(f"rank(s) {hung} still alive after {limit_s} s: killed\n" + "\n".join(errors), pytrace=False)
    if errors:
        pytest.fail("\n".join(errors), pytrace=False)
    codes = [p.exitcode for p in procs]
    assert codes == [0] * world, f"exit codes by rank: {codes}"
    return [torch.load(os.path.join(outdir, f"rank{r}.pt")) for r in range(world)]


# ---- what leaves a rank, and what one backward's buckets must satisfy ----------------------------------------------------
class RecordingReducer(GradReducer):
    """Keeps (lo, hi, copy) of every bucket in `snaps`.  The copy is queued on the compute stream in front of the
    hand-over, so it sees exactly what the all-reduce is ordered after: this rank's contribution."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.snaps = []

    def _flush(self):
        if self._pending_lo is not None:
            lo, hi = self._pending_lo, self._pending_hi
            self.snaps.append((lo, hi, self.pack.grad[lo:hi].clone()))
        super()._flush()


def assert_spans_tile(spans, total):
    """The (lo, hi) of one backward's buckets, in any order, cover [0, total) with no gap and no overlap."""
    spans = sorted(spans)
    assert spans, "no bucket left"
    assert spans[0][0] == 0, f"the buckets start at {spans[0][0]}, not 0"
    for a, b in zip(spans, spans[1:]):
        assert a[1] == b[0], f"{'gap' if a[1] < b[0] else 'overlap'} between the buckets {a} and {b}"
    assert spans[-1][1] == total, f"the buckets end at {spans[-1][1]}, the pack at {total}"


def check_tiling(reducer, pack):
    assert reducer.pack is pack, "the reducer works on another pack"
    assert_spans_tile(reducer.launched, pack.total)


def _names_in(pack, lo, hi, bad):
    """Names of the parameters of [lo, hi) that hold an element where `bad` (bool over that range) is set."""
    out = []
    for n, p, off in zip(pack.names, pack.params, pack.offsets):
        if off >= lo and off + p.numel() <= hi and bool(bad[off - lo:off - lo + p.numel()].any()):
            out.append(n)
    return out


def check_snapshots(reducer, pack):
    """Every bucket left with the values its range holds at the end of the backward (exchange over ONE rank): a gradient
    written after its bucket left, or a span reaching into a neighbour that was not finished, shows here."""
    assert reducer.snaps, "no bucket was recorded"
    for lo, hi, snap in reducer.snaps:
        final = pack.grad[lo:hi]
        if not torch.equal(snap, final):
            raise AssertionError(f"the bucket [{lo}, {hi}) left before its gradients were final: "
                                 f"{_names_in(pack, lo, hi, snap != final)}")


def assemble(reducer, total):
    """The snapshots of one backward as one flat buffer (NaN where no bucket covered)."""
    out = torch.full((total,), float("nan"), dtype=torch.float32, device=reducer.snaps[0][2].device)
    for lo, hi, snap in reducer.snaps:
        out[lo:hi] = snap
    return out


# ---- the tiny models ----------------------------------------------------------------------------------------------------
MODELS = ("vit", "vit-cls", "cait", "swin", "head")
COMPUTES = ("fp32", "bf16")
PER_RANK = 8


def ready_calls(name, model):
    """How often one backward of the model announces a section (the `_ready` sites of vit.py, cait.py and swin.py and
    the head's one hand-over), from the model's depths: with `min_bucket_elems=1` each is a bucket of its own."""
    if name in ("vit", "vit-cls"):
        return 1 + len(model.blocks) + 1                                    # norm + head | each block | embeddings
    if name == "cait":      # norm + head | class-attention blocks | trunk blocks | embeddings
        return 1 + len(model.blocks_token_only) + len(model.blocks) + 1
    if name == "swin":      # norm + head | every stage's blocks | the PatchMerging between two stages | patch embedding
        return 1 + sum(len(l.blocks) for l in model.layers) + sum(l.downsample is not None for l in model.layers) + 1
    return 1                # the stand-alone head: everything, after its backward


def _vit(compute, cls_only=False):
    from vit_torch_amd import VisionTransformer
    return VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=3, num_heads=2, num_classes=10,
                             cls_only_last_block=cls_only, compute_dtype=compute, residual_dtype="auto")


def image_size(name):
    return 56 if name == "swin" else 32


def build_case(name, compute, seed):
    """(model to train, frozen backbone in front of it or None), on the GPU, initialised from `seed` (the frozen
    backbone from a seed of its own: it is the same on every rank)."""
    torch.manual_seed(seed)
    bottom = None
    if name == "vit":
        m = _vit(compute)
    elif name == "vit-cls":
        m = _vit(compute, cls_only=True)
    elif name == "cait":
        from test_golden_gpu import cait_tiny_model
        m = cait_tiny_model(compute)
    elif name == "swin":
        from test_golden_gpu import swin_tiny_model
        m = swin_tiny_model(compute)             # drop_path_rate 0.0: random drops would differ between the ranks
    elif name == "head":
        from vit_torch_amd import VisionModelZoo
        m = VisionModelZoo.get_classifier_head(128, [32, 10])
        torch.manual_seed(7)
        bottom = _vit(compute).requires_grad_(False).cuda()
    else:
        raise ValueError(name)
    return m.cuda(), bottom


def shard(name, rank):
    """Rows [8 rank, 8 rank + 8) of the seeded batch: images on the GPU, labels on the GPU."""
    g = torch.Generator("cpu").manual_seed(0)
    s = image_size(name)
    X = torch.randn(PER_RANK * 2, 3, s, s, generator=g)
    Y = torch.randint(0, 10, (PER_RANK * 2,), generator=g)
    return X[PER_RANK * rank:PER_RANK * (rank + 1)].cuda(), Y[PER_RANK * rank:PER_RANK * (rank + 1)].cuda()


def pack_of(model):
    return model.engine().pack


def backward_once(model, bottom, x, y, reducer=None):
    """One forward and backward from cleared gradients, with `reducer` (or none) on the engine / the head; returns the
    pack after a synchronize."""
    from vit_torch_amd import CrossEntropyLoss
    eng = model.engine()
    eng.reducer = reducer
    for p in model.parameters():
        p.grad = None
    if bottom is not None:
        with torch.no_grad():
            x = bottom(x)
    CrossEntropyLoss()(model(x), y).backward()
    torch.cuda.synchronize()
    return eng.pack


def record(net, min_bucket_elems=1):
    """Replace a Network's reducer by a RecordingReducer over the same pack (Network builds it with the default
    bucket size, at which a tiny model is one bucket)."""
    eng = net.model.engine()
    net.reducer = eng.reducer = RecordingReducer(eng.pack, group=net.reducer.group, min_bucket_elems=min_bucket_elems, force=net.reducer.force)
    return net.reducer
