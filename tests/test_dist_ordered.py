"""The rank-ordered gradient exchange of GradBucketReducer (stcat_amd/dist.py; `ordered=True`, STCAT_DP_ORDERED, automatic
in deterministic mode beyond two ranks): all_to_all_single -> stcat_rank_sum -> all_gather_into_tensor per bucket, so the
cross-rank mean is the chain ((g0 + g1) + g2 ...) * fp32(1 / world) on every rank, bit for bit.

CPU: gloo over CPU tensors with the host emulator's build of the kernel, worlds 3 and 4.  GPU: RCCL at one rank (the real
asynchronous call sequence on the exchange stream), three gloo ranks sharing the card (Toy model, then the whole model in
deterministic mode).  Every comparison of exchanged gradients is torch.equal."""
import os
import queue as _queue
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from stcat_amd import _lib as L
from stcat_amd.dist import GradBucketReducer, live_trainable
from tests.test_dist import Toy, ToyEarly, _free_port

QUEUE_S, JOIN_S = 600, 120


def _run_ranks(target, world, *args):
    """start `world` workers target(rank, world, port, q, *args) and collect one result from each: 600 s for the results,
    120 s to join; a worker that dies (or the deadline) ends the others before the test fails.  Nothing is retried."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    out, failure = [], None
    deadline = time.monotonic() + QUEUE_S
    try:
        while len(out) < world and failure is None:
            try:
                out.append(q.get(timeout=0.5))
            except _queue.Empty:
                dead = [(i, p.exitcode) for i, p in enumerate(procs) if p.exitcode not in (None, 0)]
                if dead:
                    failure = f"worker (rank, exit code) {dead} failed"
                elif time.monotonic() > deadline:
                    failure = f"no result from every rank within {QUEUE_S} s"
        if failure is None:
            for i, p in enumerate(procs):
                p.join(timeout=JOIN_S)
                if p.exitcode != 0:
                    failure = f"rank {i}: exit code {p.exitcode}"
                    break
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=10)
    assert failure is None, failure
    return sorted(out, key=lambda t: t[0])


def _input(rank, step, dev="cpu"):
    """a different clip per rank and step, magnitudes mixed over seven decades (so are the gradients)"""
    g = torch.Generator().manual_seed(1000 + 10 * step + rank)
    x = torch.randn(2, 8, 5, 5, generator=g) * 10.0 ** torch.randint(-3, 4, (2, 8, 1, 1), generator=g).float()
    return x.to(dev)


def _chain(gs, world, order=None):
    order = list(range(world) if order is None else order)
    acc = gs[order[0]].clone()
    for k in order[1:]:
        acc = acc + gs[k]
    return acc * torch.tensor(np.float32(1.0 / world))


def _init(rank, world, port, backend="gloo"):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group(backend, rank=rank, world_size=world)


def _count_calls():
    """count the library calls by name (dist.py reaches the library through _lib.call)"""
    counts, orig = {}, L.call

    def call(name, *a):
        counts[name] = counts.get(name, 0) + 1
        return orig(name, *a)
    L.call = call
    return counts


def _named_grads(model):
    return {n: p.grad.detach().cpu().clone().numpy() for n, p in live_trainable(model.named_parameters())}


# ---- CPU: gloo, emulator, worlds 3 and 4 ---------------------------------------------------------------------------
def _worker_cpu(rank, world, port, q, ordered_arg):
    torch.set_num_threads(1)
    from stcat_amd import ops
    from tests.backends import use_emu
    use_emu()
    _init(rank, world, port)
    counts = _count_calls()
    res = {}
    for cls in (Toy, ToyEarly):
        torch.manual_seed(0)
        model = cls()
        red = GradBucketReducer(model, bucket_mb=0.002, extra_numel=100, ordered=ordered_arg)   # ~2 KB buckets + padded tails
        assert red.ordered is True and len(red.buckets) >= 2 and ops.GRAD_SINK is red
        assert any(b["padded"] > b["numel"] for b in red.buckets) and all(b["padded"] % (64 * world) == 0 for b in red.buckets)
        assert all(b["recv"].numel() == b["padded"] for b in red.buckets)
        got = []
        for step in range(2):                    # the second step: zero_grad() and the reuse of flat / recv
            red.zero_grad()
            model(_input(rank, step)).square().sum().backward()
            red.finish()
            got.append(_named_grads(model))
        if cls is ToyEarly:
            assert model.took == [True, True]
        red.close()                              # the plain gradients: the same backward passes with no exchange
        red.deferred = True
        local = []
        for step in range(2):
            for p in model.parameters():
                p.grad = None
            model(_input(rank, step)).square().sum().backward()
            local.append(_named_grads(model))
        res[cls.__name__] = (local, got, len(red.buckets) + 1)
    # one stcat_rank_sum per bucket and one for the dummy message, per step and model — and no 1 / world pass after it
    assert counts.get("stcat_rank_sum") == 2 * sum(r[2] for r in res.values()), counts
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def _check_exact(out, world, reversed_differs):
    for cls in ("Toy", "ToyEarly"):
        differs = False
        for step in range(2):
            local = [{n: torch.from_numpy(g) for n, g in o[1][cls][0][step].items()} for o in out]
            for n in local[0]:
                want = _chain([l[n] for l in local], world)
                differs |= not torch.equal(want, _chain([l[n] for l in local], world, reversed(range(world))))
                for rank, res in out:
                    got = torch.from_numpy(res[cls][1][step][n])
                    assert torch.equal(got, want), (cls, step, rank, n, int((got != want).sum()))
        if reversed_differs:
            assert differs, "the gradients do not tell the rank order apart: change the inputs"


@pytest.mark.parametrize("world", [3, 4])
def test_ordered_exchange_gloo_is_the_rank_chain(world):
    """every rank, every parameter, two steps, Toy and ToyEarly (early delivery): the exchanged gradient is bitwise the
    chain over the ranks' plain gradients, rank 0 first, times fp32(1 / world).  World 3: the reversed chain gives other
    bits somewhere, so a summing collective's own order cannot pass."""
    from tests.backends import use_emu
    use_emu()                                    # (builds the emulator library once, before the workers bind it)
    out = _run_ranks(_worker_cpu, world, True)
    assert [o[0] for o in out] == list(range(world))
    _check_exact(out, world, reversed_differs=(world == 3))


# ---- selection rules ---------------------------------------------------------------------------------------------------
def _worker_rules3(rank, world, port, q):
    torch.set_num_threads(1)
    from tests.backends import use_emu
    use_emu()
    _init(rank, world, port)
    seen = {}
    try:
        os.environ.pop("STCAT_DP_ORDERED", None)
        L.set_deterministic(True)
        seen["mode on"] = GradBucketReducer(Toy()).ordered
        seen["mode on, ordered=False"] = GradBucketReducer(Toy(), ordered=False).ordered
        os.environ["STCAT_DP_ORDERED"] = "0"
        seen["mode on, env 0"] = GradBucketReducer(Toy()).ordered
        L.set_deterministic(False)
        os.environ.pop("STCAT_DP_ORDERED")
        red = GradBucketReducer(Toy())
        seen["mode off"] = red.ordered
        seen["mode off: recv"] = all(b["recv"] is None for b in red.buckets)
        os.environ["STCAT_DP_ORDERED"] = "1"
        seen["mode off, env 1"] = GradBucketReducer(Toy()).ordered
        seen["mode off, env 1, ordered=False"] = GradBucketReducer(Toy(), ordered=False).ordered
        os.environ["STCAT_DP_ORDERED"] = "yes"
        try:
            GradBucketReducer(Toy())
            seen["bad env"] = "accepted"
        except ValueError as e:
            seen["bad env"] = "STCAT_DP_ORDERED" in str(e)
    finally:
        L.set_deterministic(False)
        os.environ.pop("STCAT_DP_ORDERED", None)
    q.put((rank, seen))
    dist.barrier()
    dist.destroy_process_group()


def test_ordered_selection_rules_world3():
    from tests.backends import use_emu
    use_emu()
    out = _run_ranks(_worker_rules3, 3)
    want = {"mode on": True, "mode on, ordered=False": False, "mode on, env 0": False, "mode off": False, "mode off: recv": True,
            "mode off, env 1": True, "mode off, env 1, ordered=False": False, "bad env": True}
    for rank, seen in out:
        assert seen == want, (rank, seen)


def _worker_world2(rank, world, port, q):
    torch.set_num_threads(1)
    _init(rank, world, port)
    os.environ.pop("STCAT_DP_ORDERED", None)
    os.environ["STCAT_DETERMINISTIC"] = "1"      # even with the mode asked for: two ranks have one order
    red = GradBucketReducer(Toy())
    nothing_set = (red.ordered, L._lib is None, red.collective, all(b["recv"] is None for b in red.buckets))
    red.close()
    os.environ.pop("STCAT_DETERMINISTIC")
    from tests.backends import use_emu
    use_emu()
    torch.manual_seed(0)
    model = Toy()
    red = GradBucketReducer(model, bucket_mb=0.002, ordered=True)
    red.zero_grad()
    model(_input(rank, 0)).square().sum().backward()
    red.finish()
    got = _named_grads(model)
    red.close()
    red.deferred = True
    for p in model.parameters():
        p.grad = None
    model(_input(rank, 0)).square().sum().backward()
    q.put((rank, nothing_set, red.ordered, _named_grads(model), got))
    dist.barrier()
    dist.destroy_process_group()


def test_ordered_world2_only_on_request():
    """world 2 with nothing set: off, and the constructor has not loaded the kernel library; ordered=True works there and
    gives (g0 + g1) * 0.5 exactly"""
    from tests.backends import use_emu
    use_emu()
    out = _run_ranks(_worker_world2, 2)
    for rank, nothing_set, asked, local, got in out:
        assert nothing_set == (False, True, "allreduce", True), (rank, nothing_set)
        assert asked is True
    for n in out[0][3]:
        want = (torch.from_numpy(out[0][3][n]) + torch.from_numpy(out[1][3][n])) * 0.5
        for o in out:
            assert torch.equal(torch.from_numpy(o[4][n]), want), (o[0], n)


# ---- launch plans: what a host action launches is not recorded -----------------------------------------------------------
def _worker_plan(rank, world, port, q):
    torch.set_num_threads(1)
    from stcat_amd import ops, plans
    from tests.backends import use_emu
    dev = use_emu()
    _init(rank, world, port)
    model = Toy()
    red = GradBucketReducer(model, bucket_mb=64.0, force_comm=True, ordered=True)
    assert red.ordered and red.comm and len(red.buckets) == 1
    params = [p for _, p in red.buckets[0]["params"]]
    grads = [torch.randn(p.shape).contiguous() for p in params]
    names, add_call = [], plans.Recorder.add_call

    def logged(self, name, args):
        names.append(name)
        return add_call(self, name, args)
    plans.Recorder.add_call = logged
    counts = _count_calls()
    a, b, o = torch.ones(64), torch.ones(64), torch.zeros(64)

    def ew():
        L.call("stcat_ew", L.EW_ADD, a.data_ptr(), b.data_ptr(), None, o.data_ptr(), 64, 64, 0.0, 0.0, L.stream_of(o))

    def body():                                  # a node's backward: a launch, the hand-over of its gradients, a launch
        ew()
        took = ops.host_call(lambda: red.early(params, grads))
        assert L.RECORDER is not None            # recording goes on behind the host action
        ew()
        return took
    red.zero_grad()
    took, plan = plans._record(dev, [a, b, o], None, body)
    red.finish()
    same = all(torch.equal(p.grad.reshape(-1), g.reshape(-1)) for p, g in zip(params, grads))   # the mean over one rank
    q.put((rank, bool(took), plan is not None, list(names), counts.get("stcat_rank_sum", 0), same))
    dist.barrier()
    dist.destroy_process_group()


def test_recorded_backward_does_not_hold_the_rank_sum():
    """a recorded backward whose host action (Recorder.host_call: the reducer's bucket delivery) completes a bucket with a
    live group and ordered=True: stcat_rank_sum ran (from the action), and the plan holds the node's own launches only — a
    baked copy would run at every replay beside the action's own, racing the all-to-all that fills its input"""
    from tests.backends import use_emu
    use_emu()
    (rank, took, recorded, names, n_sum, same), = _run_ranks(_worker_plan, 1)
    assert took and recorded and same
    assert n_sum == 1
    assert names == ["stcat_ew", "stcat_ew"], names


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _capture_plain(model, into):
    """the gradients autograd accumulates, cloned as they arrive (before finish() points .grad at the exchanged bucket):
    exactly what went into the exchange, whatever the backward kernels' own run-to-run behaviour"""
    for n, p in live_trainable(model.named_parameters()):
        p.register_post_accumulate_grad_hook(lambda p, n=n: into.__setitem__(n, p.grad.detach().clone()))


def _worker_gpu_toy(rank, world, port, q, backend):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    if backend == "nccl":
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        from stcat_amd.dist import init_rccl_process_group
        init_rccl_process_group(dev, rank=rank, world_size=world)
    else:
        _init(rank, world, port)
    counts = _count_calls()
    torch.manual_seed(0)
    model = Toy().to(dev)
    red = GradBucketReducer(model, bucket_mb=0.002, extra_numel=1000, force_comm=True, ordered=True)
    assert red.ordered and len(red.buckets) >= 2
    plain = {}
    _capture_plain(model, plain)
    local, got = [], []
    for step in range(2):
        red.zero_grad()
        model(_input(rank, step, dev)).square().sum().backward()
        red.finish()
        torch.cuda.synchronize()
        got.append(_named_grads(model))
        local.append({n: g.cpu().numpy() for n, g in plain.items()})
        plain.clear()
    ex = red._exchange_stream
    assert ex.priority < 0 and ex.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    assert counts.get("stcat_rank_sum") == 2 * (len(red.buckets) + 1), counts
    q.put((rank, {"Toy": (local, got)}))
    dist.barrier()
    dist.destroy_process_group()


def _check_exact_toy(out, world):
    for step in range(2):
        local = [{n: torch.from_numpy(g) for n, g in o[1]["Toy"][0][step].items()} for o in out]
        assert len(local[0]) == 3
        for n in local[0]:
            want = _chain([l[n] for l in local], world)
            for rank, res in out:
                got = torch.from_numpy(res["Toy"][1][step][n])
                assert torch.equal(got, want), (step, rank, n, int((got != want).sum()))


@pytest.mark.gpu
def test_gpu_ordered_exchange_rccl_single_rank():
    """RCCL at world size 1 (what a one-GPU box can run of the product path) with ordered=True: the real asynchronous
    sequence all_to_all_single -> stcat_rank_sum -> all_gather_into_tensor (in place in the rank's slice) on the
    high-priority exchange stream, the dummy message included.  The mean over one rank with scale 1 is a copy: the
    gradients are bitwise the plain ones."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = _run_ranks(_worker_gpu_toy, 1, "nccl")
    _check_exact_toy(out, 1)


@pytest.mark.gpu
def test_gpu_ordered_exchange_three_gloo_ranks():
    """three gloo ranks sharing the card, device tensors, the HIP library: the exactness check of the CPU test"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = _run_ranks(_worker_gpu_toy, 3, "gloo")
    _check_exact_toy(out, 3)
    local = [{n: torch.from_numpy(g) for n, g in o[1]["Toy"][0][0].items()} for o in out]
    assert any(not torch.equal(_chain([l[n] for l in local], 3), _chain([l[n] for l in local], 3, (2, 1, 0))) for n in local[0])


def _worker_model_counted(rank, world, port, q):
    """tests/test_deterministic.py::_rank_worker at any world size, with the number of stcat_rank_sum calls appended to
    its result (rank, digest, tensors, worst error, its name)"""
    from tests.test_deterministic import _rank_worker
    os.environ.pop("STCAT_DP_ORDERED", None)
    counts = _count_calls()

    class Q:
        def put(self, item):
            q.put(tuple(item) + (counts.get("stcat_rank_sum", 0),))
    _rank_worker(rank, world, port, Q(), True)


@pytest.mark.gpu
def test_gpu_deterministic_three_ranks():
    """the harness of tests/test_deterministic.py::test_gpu_deterministic_two_ranks[True] (C1, eval mode, bf16x6p, gloo,
    three steps: eager, recorded, REPLAYED from the launch plans — the backbone's hand-over is a plan yield) at world 3,
    mode on and nothing else set, so the reducer chooses the ordered exchange itself.  Run twice: SHA-256 over every reduced
    gradient is equal between the runs and across the three ranks, each rank is within that harness's 1e-2 relative-L2
    bar of the single-process mean of the three videos, and no node's recording was refused (asserted by the worker)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    runs = [_run_ranks(_worker_model_counted, 3) for _ in range(2)]
    for out in runs:
        assert [o[0] for o in out] == [0, 1, 2]
        for rank, digest, count, worst, name, n_sum in out:
            assert count > 500
            assert worst < 1e-2, (rank, worst, name)
            assert n_sum >= 3 * 4, n_sum         # three steps, at least four buckets: the ordered exchange did run
    a, b = runs
    assert [o[1] for o in a] == [o[1] for o in b], (a, b)
    assert a[0][1] == a[1][1] == a[2][1]         # every rank holds the same bits
