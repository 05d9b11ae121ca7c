"""Gradient accumulation (AdamW.accumulate, csrc/optim.h: grad_accum_kernel, TrainStep.window): every micro-step is a
normal step — zero_grad, replayed forward / backward, gradient exchange — and the sum lives in fp32 accumulators the
optimizer owns, filled by one multi-tensor launch per micro-step: acc = (first ? g : acc + g) * scale.

1. the kernel, bitwise against the fp32 torch chain ((g1 + g2) + g3) * fp32(1/3);  2. two windows against torch.optim.AdamW
fed the averaged gradients;  3. the guards;  4. the whole model under replayed launch plans;  5. two ranks."""
import copy
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from stcat_amd import _lib as L
from stcat_amd import optim, plans, synth
from tests.backends import both, close, host_memory_slot, use_emu
from tests.test_optim import _Toy, _cfg

K = 3
THIRD = torch.tensor(1.0 / K, dtype=torch.float32)      # fp32(1/3): what the last fold multiplies by
MISALIGNED = "vis_encoder.weight"                         # 90 300 elements: the scalar path over two chunks


def _rand_grads(model, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn(p.shape, generator=g) * scale
            for n, p in model.named_parameters() if p.requires_grad and n != "unused"}


class _GradFeeder:
    """puts host gradients into p.grad in the parameter's own memory layout (channels_last for the conv weight); the
    gradient of MISALIGNED is a view one element into a larger buffer, so its address is 4 bytes off a 16-byte boundary"""

    def __init__(self, model, dev, misaligned=MISALIGNED):
        self.named = dict(model.named_parameters())
        self.dev = dev
        self.off1 = None
        if misaligned is not None:
            n = self.named[misaligned].numel()
            self.off1 = (misaligned, torch.zeros(n + 4, device=dev))

    def feed(self, grads):
        for n, g in grads.items():
            p = self.named[n]
            if self.off1 is not None and n == self.off1[0]:
                view = self.off1[1][1:1 + p.numel()].view(p.shape)
                view.copy_(g.to(self.dev))
                assert view.data_ptr() % 16 == 4
                p.grad = view
            else:
                p.grad = torch.empty_like(p).copy_(g.to(self.dev))
            assert p.grad.stride() == p.stride()


def _torch_mean(gs):
    """the kernel's chain in torch on the host: left to right, then one multiply by fp32(1 / k)"""
    acc = gs[0].clone()
    for g in gs[1:]:
        acc = acc + g
    return acc * torch.tensor(1.0 / len(gs), dtype=torch.float32)


def _run_window(opt, feeder, grads_list, **kw):
    """TrainStep.window's call sequence on hand-made gradients: k - 1 accumulate() calls, then step()"""
    for j, grads in enumerate(grads_list):
        opt.zero_grad()
        feeder.feed(grads)
        if j < len(grads_list) - 1:
            opt.accumulate()
            assert opt.accumulated == j + 1
            for n, g in grads.items():       # the fold reads p.grad and leaves it alone
                assert torch.equal(feeder.named[n].grad.cpu(), g), n
    sq = opt.step(**kw)
    assert opt.accumulated == 0
    return sq


def _check_accumulators(opt, feeder, grads_list, what):
    for n in grads_list[0]:
        p = feeder.named[n]
        acc = opt._acc[p]
        assert acc.stride() == p.stride() and acc.dtype == torch.float32, n
        want = _torch_mean([g[n] for g in grads_list])
        assert torch.equal(acc.cpu(), want), f"{what}: accumulator of {n} is not the fp32 chain bit for bit"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel, bitwise
# ---------------------------------------------------------------------------------------------------------------------
@both
def _kernel_bitwise(dev, big):
    torch.manual_seed(0)
    model = _Toy().to(dev)
    feeder = _GradFeeder(model, dev)
    opt = optim.make_optimizer(_cfg(), model)
    for g in opt.param_groups:
        g["lr"] = 0.0
        g["weight_decay"] = 0.0
    assert 1.0 / K != 0.25 and float(THIRD) == float(np.float32(1.0 / K))
    grads = [_rand_grads(model, 40 + j) for j in range(K)]
    _run_window(opt, feeder, grads)
    assert set(opt._acc) == {feeder.named[n] for n in grads[0]}
    _check_accumulators(opt, feeder, grads, "first window")
    # a window that is abandoned with a NaN in one accumulator: the next window's first fold overwrites it
    bad = _rand_grads(model, 50)
    bad["rest"][1, 7] = float("nan")
    opt.zero_grad()
    feeder.feed(bad)
    opt.accumulate()
    assert opt.accumulated == 1 and torch.isnan(opt._acc[feeder.named["rest"]]).any()
    opt.discard_accumulated()
    assert opt.accumulated == 0
    grads = [_rand_grads(model, 60 + j) for j in range(K)]
    _run_window(opt, feeder, grads)
    _check_accumulators(opt, feeder, grads, "window after a discarded one")
    # the raw entry refuses bad arguments
    lib = L.load()
    t = opt._acc_table
    args = (t.table.data_ptr(), t.chunk_tensor.data_ptr(), t.chunk_off.data_ptr())
    st = L.stream_of(feeder.named["rest"])
    assert lib.stcat_grad_accumulate(None, args[1], args[2], t.n_chunks, optim.CHUNK, 1, 1.0, st) == -1
    assert b"grad_accumulate" in lib.stcat_last_error()
    assert lib.stcat_grad_accumulate(*args, -1, optim.CHUNK, 1, 1.0, st) == -1
    assert lib.stcat_grad_accumulate(*args, t.n_chunks, 0, 1, 1.0, st) == -1
    assert lib.stcat_grad_accumulate(*args, t.n_chunks, -4, 1, 1.0, st) == -1
    assert lib.stcat_grad_accumulate(*args, 0, optim.CHUNK, 1, 1.0, st) == 0         # nothing to do
    _check_accumulators(opt, feeder, grads, "after the refused calls")


# ---------------------------------------------------------------------------------------------------------------------
# 2. two windows against torch.optim.AdamW + clip_grad_norm_ on the torch-averaged gradients
# ---------------------------------------------------------------------------------------------------------------------
WINDOW_SCALES = (10.0, 1e-4)      # norm of the mean gradient ~ 3e3 (clipped to 0.1) and ~ 3e-2 (not clipped)


def _window_grads(model, w):
    return [_rand_grads(model, 100 + K * w + j, WINDOW_SCALES[w]) for j in range(K)]


def _reference_windows(cfg, decay):
    torch.manual_seed(0)
    model = _Toy()
    ema = copy.deepcopy(model)
    named = dict(model.named_parameters())
    groups = [{"params": [named["rest"], named["unused"]]},
              {"params": [named["vis_encoder.weight"], named["vis_encoder.bias"], named["vis_encoder_conv"]],
               "lr": cfg.SOLVER.VIS_BACKBONE_LR},
              {"params": [named["text_encoder.weight"], named["text_encoder.bias"]], "lr": cfg.SOLVER.TEXT_LR},
              {"params": [named["ground_decoder.temp_decoder.weight"], named["ground_decoder.temp_decoder.bias"]],
               "lr": cfg.SOLVER.TEMP_LR}]
    opt = torch.optim.AdamW(groups, lr=cfg.SOLVER.BASE_LR, weight_decay=cfg.SOLVER.WEIGHT_DECAY)
    norms = []
    for w in range(len(WINDOW_SCALES)):
        opt.zero_grad()
        gs = _window_grads(model, w)
        for n in gs[0]:
            named[n].grad = _torch_mean([g[n] for g in gs])
        norms.append(torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.SOLVER.MAX_GRAD_NORM).item())
        opt.step()
        optim.adjust_learning_rate(cfg, opt, w, 1000)
        with torch.no_grad():
            msd = model.state_dict()
            for k, v in ema.state_dict().items():
                v.copy_(v * decay + (1.0 - decay) * msd[k])
    return model, ema, norms


@both
def _window_against_torch(dev, big):
    cfg = _cfg()
    decay = 0.9
    ref_model, ref_ema, ref_norms = _reference_windows(cfg, decay)
    assert ref_norms[0] > cfg.SOLVER.MAX_GRAD_NORM > ref_norms[1] > 0      # one window clips, one does not
    torch.manual_seed(0)
    model = _Toy().to(dev)
    ema = copy.deepcopy(model)
    opt = optim.make_optimizer(cfg, model)
    feeder = _GradFeeder(model, dev)
    for w in range(len(WINDOW_SCALES)):
        sq = _run_window(opt, feeder, _window_grads(model, w), max_grad_norm=cfg.SOLVER.MAX_GRAD_NORM, model_ema=ema,
                         ema_decay=decay, model=model)
        got = sq.sqrt().item()
        print(f"window {w}: norm of the mean gradient {got:.9g} (torch {ref_norms[w]:.9g})")
        assert abs(got - ref_norms[w]) <= 1e-5 * ref_norms[w]
        optim.adjust_learning_rate(cfg, opt, w, 1000)
    assert opt.step_count == 2
    for (n, p), (_, r) in zip(model.named_parameters(), ref_model.named_parameters()):
        close(p, r, 2e-6, "parameter " + n)
    for (n, p), (_, r) in zip(ema.named_parameters(), ref_ema.named_parameters()):
        close(p, r, 2e-6, "ema " + n)
    assert torch.equal(model.frozen.cpu(), ref_model.frozen) and torch.equal(model.unused.cpu(), ref_model.unused)
    # a window of ONE micro-step is a plain step: same launches, same bits, no accumulator is ever allocated
    outs = []
    for windowed in (False, True):
        torch.manual_seed(0)
        m = _Toy().to(dev)
        e = copy.deepcopy(m)
        o = optim.make_optimizer(cfg, m)
        f = _GradFeeder(m, dev, misaligned=None)
        kw = dict(max_grad_norm=cfg.SOLVER.MAX_GRAD_NORM, model_ema=e, ema_decay=decay, model=m)
        for s in range(2):
            grads = _rand_grads(m, 200 + s, WINDOW_SCALES[s])
            if windowed:
                _run_window(o, f, [grads], **kw)
            else:
                o.zero_grad()
                f.feed(grads)
                o.step(**kw)
        assert not o._acc and o._acc_table is None and o.accumulated == 0
        outs.append([p.detach().cpu().clone() for p in list(m.parameters()) + list(e.parameters())] +
                    [o.state[p][k].cpu().clone() for p in o.state for k in ("exp_avg", "exp_avg_sq")])
    assert len(outs[0]) == len(outs[1]) and all(torch.equal(a, b) for a, b in zip(*outs))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the guards
# ---------------------------------------------------------------------------------------------------------------------
def test_emu_window_guards():
    dev = use_emu()
    cfg = _cfg()
    torch.manual_seed(0)
    model = _Toy().to(dev)
    opt = optim.make_optimizer(cfg, model)
    feeder = _GradFeeder(model, dev)
    grads = _rand_grads(model, 7)
    assert opt.accumulated == 0
    with pytest.raises(AttributeError):
        opt.accumulated = 3                              # read-only
    opt.zero_grad()
    feeder.feed(grads)
    opt.accumulate()
    assert opt.accumulated == 1
    # a micro-step that lacks one gradient, and one that has an extra one: both name the parameter
    opt.zero_grad()
    feeder.feed({n: g for n, g in grads.items() if n != "text_encoder.bias"})
    with pytest.raises(ValueError, match=r"text_encoder\.bias"):
        opt.accumulate()
    with pytest.raises(ValueError, match=r"text_encoder\.bias"):
        opt.step()
    assert opt.accumulated == 1 and opt.step_count == 0
    feeder.feed(grads)
    model.unused.grad = torch.zeros_like(model.unused)
    with pytest.raises(ValueError, match="unused"):
        opt.accumulate()
    model.unused.grad = None
    opt.accumulate()
    assert opt.accumulated == 2
    with pytest.raises(RuntimeError, match="accumulation window"):
        opt.state_dict()
    opt.discard_accumulated()
    assert opt.accumulated == 0
    sd = opt.state_dict()                                # closed window: checkpoints as before
    opt.accumulate()
    assert opt.accumulated == 1
    opt.load_state_dict(sd)
    assert opt.accumulated == 0
    # a parameter list without names still says which parameter
    plain = optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    plain.accumulate()
    model.text_encoder.bias.grad = None
    with pytest.raises(ValueError, match=r"shape \(5,\)"):
        plain.accumulate()
    # the two refusals that used to send accumulation to the slow paths name the method now
    import inspect
    from stcat_amd import dist as sdist
    assert "AdamW.accumulate()" in inspect.getsource(plans) and "AdamW.accumulate()" in inspect.getsource(sdist.GradBucketReducer.early)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the whole model under replayed launch plans
# ---------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b, what, tol):
    """tests/test_plans.py::_rel_l2 (per-tensor relative L2 with a 2e-6-per-element floor)"""
    err = (a.double() - b.double()).norm().item() / (b.double().norm().item() + 2e-6 * b.numel() ** 0.5 / tol)
    assert err <= tol, f"{what}: rel-L2 {err:.3e}"


def _model_window(dev, det, pipeline):
    """two warm-up steps (eager, recorded), plain replayed steps on clips A and B, then window(k = 2) on A, B with every
    learning rate at 0: the accumulators hold (gA + gB) * 0.5 and every node of both micro-steps was replayed"""
    from stcat_amd import backbone
    from stcat_amd.harness import TrainStep
    from tests.test_plans import _clip
    cpu = dev.type == "cpu"
    T, res = (2, 32) if cpu else (8, 224)
    L.set_mma_mode("f32" if cpu else "bf16x6p")
    L.set_deterministic(det)
    plans.clear()
    plans.enable(True)
    plans.STATS.update(recorded=0, replayed=0, eager=0, run_s=0.0, refused=0)
    saved = backbone.BLOCKS
    if cpu:
        backbone.BLOCKS = (1, 1, 2, 1)          # (tests/test_plans.py::_build: keeps the emulator run in minutes)
    ts = None
    try:
        clips = [_clip(torch.device("cpu"), T, res, k) for k in (0, 2)]
        try:
            ts = TrainStep(dev, (T, res, 5 if cpu else 10), train=False, clips=[(c.tensors, c.mask) for c in clips],
                           arena_elems=(1 << 22) if cpu else 120_000_000, pipeline_prefix=pipeline)
        finally:
            backbone.BLOCKS = saved
        opt = optim.AdamW([p for p in ts.model.parameters() if p.requires_grad], lr=0.0, weight_decay=0.0)
        names = {p: n for n, p in ts.model.named_parameters()}
        ts.step()
        ts.step()
        counts, plain = [], []
        for _ in range(2):
            before = plans.STATS["replayed"]
            ts.step()
            counts.append(plans.STATS["replayed"] - before)
            plain.append({n: g.clone() for n, g in ts.gradients().items()})
        gA, gB = plain
        n_nodes = counts[1]
        assert n_nodes >= 8 and (pipeline or counts[0] == n_nodes), counts
        assert any(not torch.equal(gA[n], gB[n]) for n in gA)
        before = dict(plans.STATS)
        taken = ts.model.vis_encoder[0].prefix_stats.get("taken", 0) if pipeline else 0
        totals, sq = ts.window(opt, 2, max_grad_norm=0.1)
        after = dict(plans.STATS)
        if pipeline:
            assert after["replayed"] - before["replayed"] >= 2 * n_nodes, (before, after, n_nodes)
            assert ts.model.vis_encoder[0].prefix_stats["taken"] == taken + 2
        else:
            assert after["replayed"] - before["replayed"] == 2 * n_nodes, (before, after, n_nodes)
            assert after["recorded"] == before["recorded"], (before, after)
        assert after["eager"] == before["eager"] and not after.get("refused"), (before, after)
        assert len(totals) == 2 and totals[0].data_ptr() != totals[1].data_ptr() and float(totals[0]) != float(totals[1])
        assert opt.accumulated == 0 and opt.step_count == 1
        assert {names[p] for p in opt._acc} == set(gA)
        norm2 = 0.0
        for p, acc in opt._acc.items():
            n = names[p]
            want = (gA[n] + gB[n]) * 0.5
            if det:
                assert torch.equal(acc, want), f"accumulator of {n} differs from (gA + gB) * 0.5"
            else:
                _rel_l2(acc.cpu(), want.cpu(), "accumulator of " + n, 3e-3)
            norm2 += float(acc.double().pow(2).sum())
        got = float(sq)
        print(f"window squared norm {got:.9g}, accumulators' {norm2:.9g}")
        assert abs(got ** 0.5 - norm2 ** 0.5) <= 1e-5 * norm2 ** 0.5
        for p in opt._acc:                                  # every learning rate is 0: the weights did not move
            assert torch.isfinite(p).all()
    finally:
        backbone.BLOCKS = saved
        plans.enable(False)
        if ts is not None:
            ts.close()
        plans.clear()
        L.set_deterministic(False)
        L.set_mma_mode("f32")


def test_emu_model_window_under_replayed_plans():
    dev = use_emu()
    with host_memory_slot():
        _model_window(dev, True, False)


@pytest.mark.gpu
def test_gpu_model_window_under_replayed_plans():
    from tests.backends import use_hip
    _model_window(use_hip(), True, False)


@pytest.mark.gpu
def test_gpu_model_window_default_mode_pipelined_prefix():
    """mode off, and every micro-step declares the next clip's frozen prefix (TrainStep(pipeline_prefix=True)): the
    run-to-run bar of tests/test_plans.py — per-tensor rel-L2 3e-3 with its 2e-6-per-element floor"""
    from tests.backends import use_hip
    _model_window(use_hip(), False, True)


# ---------------------------------------------------------------------------------------------------------------------
# 5. two ranks
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    """tests/test_dp_model.py::_worker with a window of two clips per rank (seeds 100 + 2 * rank + j): every micro-step
    exchanges as a normal step, the fold reads the bucket views after finish()"""
    import torch.distributed as dist
    from stcat_amd.dist import GradBucketReducer
    from stcat_amd.misc import BoxList, NestedTensor
    from stcat_amd.pipeline import SyntheticText, build_model
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    L.load()
    L.set_mma_mode("bf16x6p")
    T, res, Lt = synth.CONFIGS["C1"]
    model, criterion, wd = build_model(None, SyntheticText(synth.synth_text(Lt)))
    synth.fill_module_(model)
    model.to(dev).eval()

    def step(seed):
        frames = synth.synth_frames(T, res, seed=seed).to(dev)
        videos = NestedTensor(frames, torch.zeros(T, res, res, dtype=torch.bool, device=dev), [T])
        act, tb = synth.synth_targets(T, seed=seed)
        targets = [{"actioness": act.to(dev), "boxs": BoxList(tb).to(dev)}]
        plan = criterion.plan(targets, [T], dev)
        plan._num_boxes = max(plan.num_boxes_local, 1.0)      # every clip holds the same number of boxes
        out = model(videos, ["synthetic"])
        criterion(out, targets, [T], plan=plan)
        criterion.weighted_total(wd).backward()

    red = GradBucketReducer(model)
    opt = optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=0.0, weight_decay=0.0)
    names = {p: n for n, p in model.named_parameters()}
    plans.enable(True)
    for _ in range(2):                       # eager, recorded
        red.zero_grad()
        step(100 + rank)
        red.finish()
    before = dict(plans.STATS)
    micro = []
    for j in range(2):                       # the window: both micro-steps REPLAYED, exchanged, folded
        red.zero_grad()
        step(100 + 2 * rank + j)
        red.finish()
        micro.append({names[p]: p.grad.detach().clone() for p in opt._plist if p.grad is not None})
        if j == 0:
            opt.accumulate()
    opt.step()
    torch.cuda.synchronize()
    # the fold itself, apart from the exchange: bit for bit the chain over what finish() left in the bucket views
    assert len(micro[0]) == len(opt._acc)
    for p, a in opt._acc.items():
        assert torch.equal(a, (micro[0][names[p]] + micro[1][names[p]]) * 0.5), names[p]
    replayed = plans.STATS["replayed"] - before["replayed"]
    assert plans.STATS["eager"] == before["eager"] and not plans.STATS.get("refused"), (before, plans.STATS)
    plans.enable(False)
    got = {names[p]: a.detach().clone() for p, a in opt._acc.items()}
    # single-process reference: the four clips, no exchange
    red.close()
    red.deferred = True
    ref = {}
    for s in range(2 * world):
        for p in model.parameters():
            p.grad = None
        step(100 + s)
        for n, p in model.named_parameters():
            if p.grad is not None:
                ref[n] = ref.get(n, 0) + p.grad.detach() / (2 * world)
    assert set(got) == set(ref)
    # tests/test_dp_model.py's scale rule: relative to max(|ref|, the typical gradient magnitude), in the L2 norm
    typical = float(torch.stack([ref[n].norm() / ref[n].numel() ** 0.5 for n in ref]).median())
    worst, worst_n = 0.0, ""
    for n in ref:
        scale = max(float(ref[n].norm()), typical * ref[n].numel() ** 0.5)
        err = float((got[n] - ref[n]).norm()) / scale
        if err > worst:
            worst, worst_n = err, n
    # the ranks hold the same reduced bits, so their accumulators agree bit for bit: one number to compare across ranks
    sig = float(sum(g.double().sum() for g in got.values()))
    ref_sig = float(sum(g.double().sum() for g in ref.values()))
    print(f"rank {rank}: worst {worst_n} {worst:.3e} |got| {float(got[worst_n].norm()):.6e} |ref| {float(ref[worst_n].norm()):.6e} "
          f"sum(got) {sig!r} sum(ref) {ref_sig!r}", flush=True)
    q.put((rank, worst, worst_n, replayed, len(got), sig))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_gpu_two_rank_window_equals_single_process_mean_c1():
    """two ranks x two clips: the mean of the per-micro-step rank means is the mean over the four clips.
    Measured on one MI355X: worst tensor 1.2e-5 .. 1.4e-5 on both ranks in four of five runs (alone and inside the whole
    GPU suite).  One run inside the whole suite missed the bar on rank 1 alone — vis_encoder.0.body.layer3.2.conv3.weight
    at 1.345e-1 while rank 0 stood at 2.8e-6 — and did not come back; its cause was not found.  The worker has since
    checked the fold against what finish() left in the bucket views bit for bit, and the test compares the ranks'
    accumulators with each other, so a repeat says whether the exchange, the fold or the single-process reference moved."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert out[0][5] == out[1][5], ("the ranks' accumulators differ", out[0][5], out[1][5])
    for rank, worst, name, replayed, n_grads, _ in out:
        print(f"rank {rank}: worst tensor {name}: {worst:.3e}; {replayed} node replays in the window")
        assert replayed >= 20 and n_grads > 500, (replayed, n_grads)
        # not bitwise (atomically ordered split-K sums, ReLU-kink flips): a missing, doubled or unscaled micro-step or
        # rank contribution would be an O(1) error
        assert worst < 1e-2, (rank, worst, name)
